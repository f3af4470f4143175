// BoomerAMG setup (HYPRE_BoomerAMGSetup, reached from src/HypreSystem.cpp:692
// through HYPRE_ParCSRGMRESSetup).  Host control plane, threaded over rows;
// outside the solve-phase metric.  Algorithms per SURVEY A.5:
// strength (par_strength.c), PMIS (par_coarsen.c), extended+i / direct /
// classical-modified interpolation with truncation (par_lr_interp.c,
// par_interp.c), Galerkin R*(A*P) (par_rap.c), l1 norms (par_relax_more.c).
//
// Multi-rank variant: coarsening and interpolation are rank-local (connections
// to halo columns are treated as weak), so P has no off-rank columns and the
// Galerkin product needs exactly one exchange: the P rows of the halo columns.
#include <algorithm>
#include <atomic>
#include <thread>
#include <cmath>
#include <climits>
#include <cstring>
#include <mutex>

#include "amg.hpp"
#include "amg_setup_internal.hpp"
#include "kernels.hpp"
#include "solvers.hpp"

namespace mi {

namespace hs {  // host setup algorithms, shared with amg_setup_dist.cpp (amg_setup_internal.hpp)

constexpr int MAX_DENSE = 4096;

// strong iff a_ij < theta*min_k a_ik (a_ii > 0; mirrored for a_ii < 0); the row
// scale and row sum run over diag AND offd entries; only diag-block entries are
// kept because halo connections do not take part in rank-local coarsening
void strength(const ParCSR &A, double theta, double max_row_sum, Strength &S) {
  const HostCSR &D = A.diag, &O = A.offd;
  const int n = D.nrows;
  std::vector<StrengthRule> rule((size_t)n);
  std::vector<int64_t> dpos((size_t)n, -1);  // the diagonal's entry
  S.ia.assign((size_t)n + 1, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      const int64_t r0 = D.ia[(size_t)i], r1 = D.ia[(size_t)i + 1], o0 = O.ia[(size_t)i];
      for (int64_t k = r0; k < r1; k++)
        if (D.ja[(size_t)k] == i) dpos[(size_t)i] = k;
      const int64_t dp = dpos[(size_t)i];
      const StrengthRule r = strength_rule(D.a.data() + r0, r1 - r0, dp < 0 ? -1 : dp - r0, theta, max_row_sum,
                                           O.a.data() + o0, O.ia[(size_t)i + 1] - o0);
      int64_t c = 0;
      for (int64_t k = r0; k < r1; k++) c += (k != dp && r(D.a[(size_t)k]));
      rule[(size_t)i] = r;
      S.ia[(size_t)i + 1] = c;
    }
  });
  for (int i = 0; i < n; i++) S.ia[(size_t)i + 1] += S.ia[(size_t)i];
  S.ja.resize((size_t)S.ia[(size_t)n]);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int64_t q = S.ia[(size_t)i];
      for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++)
        if (k != dpos[(size_t)i] && rule[(size_t)i](D.a[(size_t)k])) S.ja[(size_t)q++] = D.ja[(size_t)k];
    }
  });
}

void filter_same_function(const HostCSR &A, const std::vector<int> &dof, HostCSR &F) {
  const int n = A.nrows;
  F.nrows = n;
  F.ncols = A.ncols;
  F.ia.assign((size_t)n + 1, 0);
  auto kept = [&](int64_t i, int64_t k) { return A.ja[(size_t)k] == i || dof[(size_t)A.ja[(size_t)k]] == dof[(size_t)i]; };
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int64_t c = 0;
      for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) c += kept(i, k);
      F.ia[(size_t)i + 1] = c;
    }
  });
  for (int i = 0; i < n; i++) F.ia[(size_t)i + 1] += F.ia[(size_t)i];
  F.ja.resize((size_t)F.ia[(size_t)n]);
  F.a.resize((size_t)F.ia[(size_t)n]);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int64_t q = F.ia[(size_t)i];
      for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++)
        if (kept(i, k)) {
          F.ja[(size_t)q] = A.ja[(size_t)k];
          F.a[(size_t)q++] = A.a[(size_t)k];
        }
    }
  });
}

// keep entries >= trunc_factor*max|p|, then the pmax largest by (|p| desc,
// position asc), rescale to the original row sum; stored order is kept
int truncate_row(int len, int *cols, double *vals, double trunc_factor, int pmax, std::vector<char> &keep) {
  if (len == 0) return 0;
  double row_sum = 0.0, maxabs = 0.0;
  for (int k = 0; k < len; k++) {
    row_sum += vals[k];
    maxabs = std::max(maxabs, std::fabs(vals[k]));
  }
  keep.assign((size_t)len, 1);
  if (trunc_factor > 0.0)
    for (int k = 0; k < len; k++) keep[(size_t)k] = std::fabs(vals[k]) >= trunc_factor * maxabs;
  int nk = 0;
  for (int k = 0; k < len; k++) nk += keep[(size_t)k];
  if (pmax > 0)
    while (nk > pmax) {
      int worst = -1;
      for (int k = 0; k < len; k++)
        if (keep[(size_t)k] && (worst < 0 || std::fabs(vals[k]) <= std::fabs(vals[worst]))) worst = k;
      keep[(size_t)worst] = 0;
      nk--;
    }
  double kept = 0.0;
  for (int k = 0; k < len; k++)
    if (keep[(size_t)k]) kept += vals[k];
  const double scale = (kept != 0.0) ? row_sum / kept : 1.0;
  int m = 0;
  for (int k = 0; k < len; k++)
    if (keep[(size_t)k]) {
      cols[m] = cols[k];
      vals[m] = vals[k] * scale;
      m++;
    }
  return m;
}

// interpolation of the rank-local block; halo entries are lumped into the
// diagonal like weak connections
void build_interp(const ParCSR &A, const Strength &S, std::vector<int> &cf, int interp_type, double trunc_factor,
                  int pmax, HostCSR &P, int &nc_out, const std::vector<char> *want_rows) {
  const HostCSR &D = A.diag, &O = A.offd;
  const int n = D.nrows;
  std::vector<int> f2c;
  const int nc = nc_out = coarse_numbering(cf, f2c);
  RowCollector<int> rows(n);
  parallel_for(n, [&](int64_t b, int64_t e, int t) {
    auto &out = rows.begin(t, b);
    std::vector<int> rc, sf;  // interpolatory set (fine ids, discovery order), strong F neighbours
    std::vector<double> rv;
    std::vector<char> keep;
    auto find = [](const std::vector<int> &v, int x) {
      for (size_t q = 0; q < v.size(); q++)
        if (v[q] == x) return (int)q;
      return -1;
    };
    for (int64_t i = b; i < e; i++) {
      rc.clear();
      rv.clear();
      sf.clear();
      if (want_rows && !(*want_rows)[(size_t)i]) {
        // a row of the extended sub-problem that belongs to another rank: left empty
      } else if (cf[(size_t)i] == C_PT) {
        rc.push_back((int)i);
        rv.push_back(1.0);
      } else if (cf[(size_t)i] != SF_PT) {
        for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1]; k++) {
          const int i1 = S.ja[(size_t)k];
          if (cf[(size_t)i1] == C_PT) {
            if (find(rc, i1) < 0) rc.push_back(i1);
          } else if (cf[(size_t)i1] != SF_PT && interp_type != 3) {
            sf.push_back(i1);
            if (interp_type == 6)
              for (int64_t kk = S.ia[(size_t)i1]; kk < S.ia[(size_t)i1 + 1]; kk++) {
                const int k1 = S.ja[(size_t)kk];
                if (cf[(size_t)k1] == C_PT && find(rc, k1) < 0) rc.push_back(k1);
              }
          }
        }
        rv.assign(rc.size(), 0.0);
        double diagonal = 0.0;
        for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++)
          if (D.ja[(size_t)k] == i) diagonal = D.a[(size_t)k];
        if (interp_type == 3) {
          double sNp = 0, sNn = 0, sPp = 0, sPn = 0;
          for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++) {
            const int j = D.ja[(size_t)k];
            if (j == i) continue;
            const double v = D.a[(size_t)k];
            (v > 0 ? sNp : sNn) += v;
            const int q = find(rc, j);
            if (q >= 0) {
              rv[(size_t)q] += v;
              (v > 0 ? sPp : sPn) += v;
            }
          }
          for (int64_t k = O.ia[(size_t)i]; k < O.ia[(size_t)i + 1]; k++) (O.a[(size_t)k] > 0 ? sNp : sNn) += O.a[(size_t)k];
          double alfa = 1.0, beta = 1.0;
          if (sPn != 0) alfa = sNn / sPn / diagonal;
          if (sPp != 0) beta = sNp / sPp / diagonal;
          if (sPp == 0) {
            const double d2 = diagonal + sNp;
            if (sPn != 0) alfa = sNn / sPn / d2;
            beta = 0.0;
          }
          for (size_t q = 0; q < rv.size(); q++) rv[q] = (rv[q] > 0) ? -beta * rv[q] : -alfa * rv[q];
        } else {
          for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++) {
            const int i1 = D.ja[(size_t)k];
            if (i1 == i) continue;
            const double aik = D.a[(size_t)k];
            const int q = find(rc, i1);
            if (q >= 0) {
              rv[(size_t)q] += aik;
            } else if (find(sf, i1) >= 0) {
              double dk = 0.0;
              for (int64_t kk = D.ia[(size_t)i1]; kk < D.ia[(size_t)i1 + 1]; kk++)
                if (D.ja[(size_t)kk] == i1) dk = D.a[(size_t)kk];
              const double sgn = (dk < 0) ? -1.0 : 1.0;
              double sum = 0.0;
              for (int64_t kk = D.ia[(size_t)i1]; kk < D.ia[(size_t)i1 + 1]; kk++) {
                const int i2 = D.ja[(size_t)kk];
                if (i2 == i1) continue;
                if ((find(rc, i2) >= 0 || (interp_type == 6 && i2 == i)) && sgn * D.a[(size_t)kk] < 0)
                  sum += D.a[(size_t)kk];
              }
              if (sum != 0.0) {
                const double distribute = aik / sum;
                for (int64_t kk = D.ia[(size_t)i1]; kk < D.ia[(size_t)i1 + 1]; kk++) {
                  const int i2 = D.ja[(size_t)kk];
                  if (i2 == i1) continue;
                  if (sgn * D.a[(size_t)kk] < 0) {
                    const int q2 = find(rc, i2);
                    if (q2 >= 0)
                      rv[(size_t)q2] += distribute * D.a[(size_t)kk];
                    else if (interp_type == 6 && i2 == i)
                      diagonal += distribute * D.a[(size_t)kk];
                  }
                }
              } else
                diagonal += aik;
            } else
              diagonal += aik;
          }
          for (int64_t k = O.ia[(size_t)i]; k < O.ia[(size_t)i + 1]; k++) diagonal += O.a[(size_t)k];
          if (diagonal != 0.0)
            for (size_t q = 0; q < rv.size(); q++) rv[q] /= -diagonal;
        }
        const int m = truncate_row((int)rc.size(), rc.data(), rv.data(), trunc_factor, pmax, keep);
        rc.resize((size_t)m);
        rv.resize((size_t)m);
      }
      // coarse column ids, ascending
      const int len = (int)rc.size();
      for (int q = 0; q < len; q++) rc[(size_t)q] = f2c[(size_t)rc[(size_t)q]];
      for (int a = 1; a < len; a++) {
        const int c = rc[(size_t)a];
        const double v = rv[(size_t)a];
        int bb = a - 1;
        while (bb >= 0 && rc[(size_t)bb] > c) {
          rc[(size_t)bb + 1] = rc[(size_t)bb];
          rv[(size_t)bb + 1] = rv[(size_t)bb];
          bb--;
        }
        rc[(size_t)bb + 1] = c;
        rv[(size_t)bb + 1] = v;
      }
      rows.len[(size_t)i] = len;
      out.j.insert(out.j.end(), rc.begin(), rc.end());
      out.a.insert(out.a.end(), rv.begin(), rv.end());
    }
  });
  P.nrows = n;
  P.ncols = nc;
  P.ia.assign(1, 0);
  rows.assemble(P.ia, P.ja, &P.a);
  if (!want_rows)
    for (int i = 0; i < n; i++)
      if (cf[(size_t)i] == SF_PT) cf[(size_t)i] = F_PT;
}

// ---- coarsening types beyond PMIS, and aggressive coarsening (mirrors oracle/oracle.c statement by statement)

// S^T: row i lists, ascending, the points that strongly depend on i
void strength_transpose(int n, const Strength &S, Strength &T) {
  T.ia.assign((size_t)n + 1, 0);
  T.ja.resize(S.ja.size());
  for (size_t k = 0; k < S.ja.size(); k++) T.ia[(size_t)S.ja[k] + 1]++;
  for (int i = 0; i < n; i++) T.ia[(size_t)i + 1] += T.ia[(size_t)i];
  std::vector<int64_t> pos(T.ia.begin(), T.ia.end() - 1);
  for (int i = 0; i < n; i++)
    for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1]; k++) T.ja[(size_t)pos[(size_t)S.ja[(size_t)k]]++] = i;
}

// bucket lists of the Ruge-Stueben first pass (hypre_enter_on_lists / hypre_remove_point): one FIFO list per
// integer measure, the next C point is the head of the highest non-empty list
struct RsLists {
  std::vector<int> head, tail, prev, next;
  int top = 0;
  RsLists(int nb, int n) : head((size_t)nb, -1), tail((size_t)nb, -1), prev((size_t)n, -1), next((size_t)n, -1) {}
  void enter(int m, int i) {
    prev[(size_t)i] = tail[(size_t)m];
    next[(size_t)i] = -1;
    if (tail[(size_t)m] >= 0)
      next[(size_t)tail[(size_t)m]] = i;
    else
      head[(size_t)m] = i;
    tail[(size_t)m] = i;
    if (m > top) top = m;
  }
  void remove(int m, int i) {
    if (prev[(size_t)i] >= 0)
      next[(size_t)prev[(size_t)i]] = next[(size_t)i];
    else
      head[(size_t)m] = next[(size_t)i];
    if (next[(size_t)i] >= 0)
      prev[(size_t)next[(size_t)i]] = prev[(size_t)i];
    else
      tail[(size_t)m] = prev[(size_t)i];
  }
};

// classical Ruge-Stueben coarsening on the (global) strength graph: hypre_BoomerAMGCoarsenRuge.  First pass by
// measure |S^T_i| with bucket lists; second pass (types 1, 3, 6): strong F-F pairs must share a C point.
// Sequential by definition -- HYPRE's device build offers PMIS only; these types exist so that inputs which ask
// for them (the upstream sample: coarsen_type 6, etc/hypre_app.yaml:35) get what they ask for.
void ruge_stueben(int n, const Strength &S, bool second_pass, std::vector<int> &cf) {
  Strength T;
  strength_transpose(n, S, T);
  std::vector<int> measure((size_t)n);
  int maxm = 0;
  for (int i = 0; i < n; i++) {
    measure[(size_t)i] = (int)(T.ia[(size_t)i + 1] - T.ia[(size_t)i]);
    maxm = std::max(maxm, measure[(size_t)i]);
  }
  RsLists q(2 * maxm + 2, n);
  cf.assign((size_t)n, 0);
  int64_t num_left = 0;
  for (int i = 0; i < n; i++) {
    if (S.ia[(size_t)i + 1] == S.ia[(size_t)i]) {
      cf[(size_t)i] = SF_PT;
      measure[(size_t)i] = 0;
    } else
      num_left++;
  }
  auto bump = [&](int p2) {  // an undecided point gains one
    q.remove(measure[(size_t)p2], p2);
    measure[(size_t)p2]++;
    q.enter(measure[(size_t)p2], p2);
  };
  for (int j = 0; j < n; j++) {
    if (cf[(size_t)j] != 0) continue;
    if (measure[(size_t)j] > 0) {
      q.enter(measure[(size_t)j], j);
    } else {
      cf[(size_t)j] = F_PT;
      num_left--;
      for (int64_t k = S.ia[(size_t)j]; k < S.ia[(size_t)j + 1]; k++) {
        const int nb = S.ja[(size_t)k];
        if (cf[(size_t)nb] != 0) continue;
        if (nb < j) {
          if (measure[(size_t)nb] > 0) q.remove(measure[(size_t)nb], nb);
          measure[(size_t)nb]++;
          q.enter(measure[(size_t)nb], nb);
        } else
          measure[(size_t)nb]++;
      }
    }
  }
  while (num_left > 0) {
    while (q.top > 0 && q.head[(size_t)q.top] < 0) q.top--;
    const int c = q.head[(size_t)q.top];
    if (c < 0) break;
    cf[(size_t)c] = C_PT;
    q.remove(measure[(size_t)c], c);
    measure[(size_t)c] = 0;
    num_left--;
    for (int64_t j = T.ia[(size_t)c]; j < T.ia[(size_t)c + 1]; j++) {
      const int nb = T.ja[(size_t)j];
      if (cf[(size_t)nb] != 0) continue;
      cf[(size_t)nb] = F_PT;
      q.remove(measure[(size_t)nb], nb);
      num_left--;
      for (int64_t k = S.ia[(size_t)nb]; k < S.ia[(size_t)nb + 1]; k++)
        if (cf[(size_t)S.ja[(size_t)k]] == 0) bump(S.ja[(size_t)k]);
    }
    for (int64_t j = S.ia[(size_t)c]; j < S.ia[(size_t)c + 1]; j++) {
      const int nb = S.ja[(size_t)j];
      if (cf[(size_t)nb] != 0) continue;
      q.remove(measure[(size_t)nb], nb);
      measure[(size_t)nb]--;
      if (measure[(size_t)nb] > 0)
        q.enter(measure[(size_t)nb], nb);
      else {
        cf[(size_t)nb] = F_PT;
        num_left--;
        for (int64_t k = S.ia[(size_t)nb]; k < S.ia[(size_t)nb + 1]; k++)
          if (cf[(size_t)S.ja[(size_t)k]] == 0) bump(S.ja[(size_t)k]);
      }
    }
  }
  if (!second_pass) return;
  std::vector<int> mark((size_t)n, -1);
  for (int i = 0; i < n; i++) {
    if (cf[(size_t)i] != F_PT) continue;
    int tentative = -1;
    for (;;) {
      for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1]; k++)
        if (cf[(size_t)S.ja[(size_t)k]] == C_PT) mark[(size_t)S.ja[(size_t)k]] = i;
      int lonely = -1;  // first strong F neighbour that shares no C point with i
      for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1] && lonely < 0; k++) {
        const int j = S.ja[(size_t)k];
        if (cf[(size_t)j] != F_PT) continue;
        bool shared = false;
        for (int64_t kk = S.ia[(size_t)j]; kk < S.ia[(size_t)j + 1]; kk++) {
          const int c = S.ja[(size_t)kk];
          if (mark[(size_t)c] == i && cf[(size_t)c] == C_PT) {
            shared = true;
            break;
          }
        }
        if (!shared) lonely = j;
      }
      if (lonely < 0) break;
      if (tentative < 0) {
        tentative = lonely;
        cf[(size_t)lonely] = C_PT;
      } else {
        cf[(size_t)i] = C_PT;
        cf[(size_t)tentative] = F_PT;
        break;
      }
    }
  }
}

bool coarsen_type_restated(int type) {
  return type == 8 || type == 9 || type == 10 || type == 11 || type == 6 || type == 1 || type == 3 || type == 0 || type == 7;
}

// The graph view of the coarsening core (amg_setup_internal.hpp) for a Strength pattern on one rank: every neighbour
// is an own row, every exchange is empty.
struct LocalGraph {
  static constexpr bool has_halo = false;
  const int nrows;
  const Strength &S;
  int n() const { return nrows; }
  int nh() const { return 0; }
  int64_t nnz() const { return (int64_t)S.ja.size(); }
  gidx first_id() const { return 0; }
  template <class F>
  bool each(int i, F f) const {
    for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1]; k++)
      if (f(k, S.ja[(size_t)k], -1)) return true;
    return false;
  }
  template <class T>
  void forward(const std::vector<T> &, std::vector<T> &) const {}
  template <class T, class F>
  void reverse(const std::vector<T> &, std::vector<T> &, F) const {}
  long long global_sum(long long v) const { return v; }
  // CLJP H2, "do rows i and j share a C point": marker form.  marks[c] == i + 1: C point c is in the row of i -- one
  // array of n per thread, no search.  (DistGraph in amg_setup_dist.cpp keeps the sorted-list form: there a C point
  // may be a halo point or a point two rings away, which has no index to mark.)
  using Marks = std::vector<int>;
  void fetch_strong_halo_rows() {}
  std::vector<Marks> make_marks() const { return std::vector<Marks>((size_t)host_threads()); }
  void begin_row(Marks &mk, int) const {
    if (mk.size() != (size_t)nrows) mk.assign((size_t)nrows, 0);
  }
  void mark(Marks &mk, int i, int64_t, int j) const { mk[(size_t)j] = i + 1; }
  bool shares(const Marks &mk, int i, int j, int) const {
    return each(j, [&](int64_t, int c, int) { return mk[(size_t)c] == i + 1; });
  }
};

// HYPRE_BoomerAMGSetCoarsenType (src/HypreSystem.cpp:125-126): 8 PMIS; 10 HMIS / 11 = one-pass Ruge-Stueben;
// 6 Falgout / 1 / 3 = two-pass Ruge-Stueben.  HMIS and Falgout finish with PMIS / CLJP on what the Ruge-Stueben
// pass leaves undecided; coarsening sees the whole graph here, where nothing is left --
// as on a single HYPRE rank.
void coarsen_by_type(int type, int n, const Strength &S, std::vector<int> &cf) {
  LocalGraph g{n, S};
  std::vector<int> no_halo;
  if (type == 8 || type == 9)  // 9 = PMIS with one global random stream: what 8 is here anyway
    pmis(g, cf, no_halo);
  else if (type == 0 || type == 7)  // 7 = CLJP with one global random stream: the only kind this library draws
    cljp(g, cf, no_halo);
  else if (type == 10 || type == 11)
    ruge_stueben(n, S, false, cf);
  else if (type == 6 || type == 1 || type == 3)
    ruge_stueben(n, S, true, cf);
  else
    fail(4, "BoomerAMG: coarsen_type " + std::to_string(type) + " is not implemented (8, 10, 11, 6, 1, 3, 0, 7 are)");
}

// hypre_BoomerAMGCreate2ndS, num_paths 1: graph on the C points of the first coarsening; C point i depends on
// C point j != i iff j is in S_i or in S_k for some k in S_i.  Coarse indices, columns ascending.
void second_strength(int n, const Strength &S, const std::vector<int> &cf, Strength &S2, int &nc_out) {
  std::vector<int> f2c;
  const int nc = nc_out = coarse_numbering(cf, f2c);
  std::vector<int> crow((size_t)nc);
  for (int i = 0; i < n; i++)
    if (f2c[(size_t)i] >= 0) crow[(size_t)f2c[(size_t)i]] = i;
  RowCollector<int> rows(nc);  // (the pattern alone)
  parallel_for(nc, [&](int64_t b, int64_t e, int t) {
    std::vector<int> &out = rows.begin(t, b).j;
    std::vector<int> row;
    for (int64_t ci = b; ci < e; ci++) {
      const int i = crow[(size_t)ci];
      row.clear();
      auto add = [&](int j) {
        const int cj = f2c[(size_t)j];
        if (cj >= 0 && cj != ci) row.push_back(cj);
      };
      for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1]; k++) {
        const int k1 = S.ja[(size_t)k];
        add(k1);
        for (int64_t kk = S.ia[(size_t)k1]; kk < S.ia[(size_t)k1 + 1]; kk++) add(S.ja[(size_t)kk]);
      }
      std::sort(row.begin(), row.end());
      row.erase(std::unique(row.begin(), row.end()), row.end());
      rows.len[(size_t)ci] = (int)row.size();
      out.insert(out.end(), row.begin(), row.end());
    }
  });
  S2.ia.assign(1, 0);
  rows.assemble(S2.ia, S2.ja);
}

// aggressive coarsening of one level (par_amg_setup.c, level < agg_num_levels; src/HypreSystem.cpp:215-219):
// coarsen with S, coarsen the C points again with the second-generation graph, keep what survives both.
// stage1 (optional): the marker after the first coarsening -- the two-stage interpolation's C1
void coarsen_aggressive(int type, int n, const Strength &S, std::vector<int> &cf, std::vector<int> *stage1 = nullptr) {
  coarsen_by_type(type, n, S, cf);
  if (stage1) *stage1 = cf;
  Strength S2;
  int nc = 0;
  second_strength(n, S, cf, S2, nc);
  std::vector<int> cf2;
  coarsen_by_type(type, nc, S2, cf2);
  int q = 0;
  for (int i = 0; i < n; i++)
    if (cf[(size_t)i] == C_PT) {
      if (cf2[(size_t)q] != C_PT) cf[(size_t)i] = cf2[(size_t)q];
      q++;
    }
}

// Multipass interpolation (hypre_BoomerAMGBuildMultipass; agg_interp_type 4, src/HypreSystem.cpp:220-224): see
// oracle/oracle.c build_multipass for the formulas.  Pass by pass; the rows of one pass are independent (threads),
// every row is accumulated by one thread in the oracle's order.
void build_multipass(const ParCSR &A, const Strength &S, std::vector<int> &cf, double trunc_factor, int pmax,
                     HostCSR &P, int &nc_out) {
  const HostCSR &D = A.diag;
  const int n = D.nrows;
  std::vector<int> f2c;
  const int nc = nc_out = coarse_numbering(cf, f2c);
  std::vector<int> assigned((size_t)n, -1), rlen((size_t)n, 0);
  std::vector<int64_t> rstart((size_t)n, 0);
  std::vector<int> pool_c;  // rows in the order they were built: coarse columns / weights in discovery order
  std::vector<double> pool_v;
  pool_c.reserve((size_t)n);
  pool_v.reserve((size_t)n);
  int64_t remaining = 0;
  for (int i = 0; i < n; i++) {
    if (cf[(size_t)i] == C_PT) {
      assigned[(size_t)i] = 0;
      rstart[(size_t)i] = (int64_t)pool_c.size();
      rlen[(size_t)i] = 1;
      pool_c.push_back(f2c[(size_t)i]);
      pool_v.push_back(1.0);
    } else if (cf[(size_t)i] != SF_PT)
      remaining++;
  }
  const int nt = host_threads();
  std::vector<std::vector<int>> cpos((size_t)nt);
  std::vector<int> list;
  for (int pass = 1; remaining > 0; pass++) {
    list.clear();
    for (int i = 0; i < n; i++) {
      if (assigned[(size_t)i] != -1 || cf[(size_t)i] == SF_PT) continue;
      for (int64_t k = S.ia[(size_t)i]; k < S.ia[(size_t)i + 1]; k++)
        if (assigned[(size_t)S.ja[(size_t)k]] == pass - 1) {
          list.push_back(i);
          break;
        }
    }
    const int64_t nl = (int64_t)list.size();
    if (nl == 0) break;
    RowCollector<int> rows(nl);
    parallel_for(nl, [&](int64_t b, int64_t e, int t) {
      std::vector<int> &pos = cpos[(size_t)t];
      if (pos.size() != (size_t)nc) pos.assign((size_t)nc, -1);
      auto &out = rows.begin(t, b);
      std::vector<int> &oc = out.j;
      std::vector<double> &ov = out.a;
      for (int64_t q = b; q < e; q++) {
        const int i = list[(size_t)q];
        const size_t base = oc.size();
        double diagonal = 0.0, sum_N = 0.0, sum_J = 0.0;
        for_each_entry_strong(D, S, i, [&](int64_t k, int j, bool strong) {
          if (j == i) {
            diagonal = D.a[(size_t)k];
            return;
          }
          sum_N += D.a[(size_t)k];
          if (!strong || assigned[(size_t)j] != pass - 1) return;
          sum_J += D.a[(size_t)k];
          const int64_t r0 = rstart[(size_t)j];
          for (int w = 0; w < rlen[(size_t)j]; w++) {
            const int c = pool_c[(size_t)(r0 + w)];
            if (pos[(size_t)c] < 0) {
              pos[(size_t)c] = (int)(oc.size() - base);
              oc.push_back(c);
              ov.push_back(0.0);
            }
            ov[base + (size_t)pos[(size_t)c]] += D.a[(size_t)k] * pool_v[(size_t)(r0 + w)];
          }
        });
        for (int64_t k = A.offd.ia[(size_t)i]; k < A.offd.ia[(size_t)i + 1]; k++) sum_N += A.offd.a[(size_t)k];
        const double alfa = (sum_J * diagonal != 0.0) ? -sum_N / (sum_J * diagonal) : 0.0;
        const int len = (int)(oc.size() - base);
        for (int w = 0; w < len; w++) {
          ov[base + (size_t)w] *= alfa;
          pos[(size_t)oc[base + (size_t)w]] = -1;
        }
        rows.len[(size_t)q] = len;
      }
    });
    // append the pass's rows to the pool (list order) -- only now do its points count as reached
    std::vector<int64_t> at(1, (int64_t)pool_c.size());
    rows.assemble(at, pool_c, &pool_v);
    for (int64_t q = 0; q < nl; q++) {
      rstart[(size_t)list[(size_t)q]] = at[(size_t)q];
      rlen[(size_t)list[(size_t)q]] = rows.len[(size_t)q];
      assigned[(size_t)list[(size_t)q]] = pass;
    }
    remaining -= nl;
  }
  // truncation and sort row by row (in place in the pool), then compaction into P
  std::vector<int> flen((size_t)n, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    std::vector<char> keep;
    for (int64_t i = b; i < e; i++) {
      int len = rlen[(size_t)i];
      int *rc = pool_c.data() + rstart[(size_t)i];
      double *rv = pool_v.data() + rstart[(size_t)i];
      if (cf[(size_t)i] != C_PT && len > 0) len = truncate_row(len, rc, rv, trunc_factor, pmax, keep);
      for (int a = 1; a < len; a++) {
        const int c = rc[a];
        const double v = rv[a];
        int bb = a - 1;
        while (bb >= 0 && rc[bb] > c) {
          rc[bb + 1] = rc[bb];
          rv[bb + 1] = rv[bb];
          bb--;
        }
        rc[bb + 1] = c;
        rv[bb + 1] = v;
      }
      flen[(size_t)i] = len;
    }
  });
  P.nrows = n;
  P.ncols = nc;
  P.ia.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) P.ia[(size_t)i + 1] = P.ia[(size_t)i] + flen[(size_t)i];
  P.ja.resize((size_t)P.nnz());
  P.a.resize((size_t)P.nnz());
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      if (!flen[(size_t)i]) continue;
      memcpy(P.ja.data() + P.ia[(size_t)i], pool_c.data() + rstart[(size_t)i], (size_t)flen[(size_t)i] * sizeof(int));
      memcpy(P.a.data() + P.ia[(size_t)i], pool_v.data() + rstart[(size_t)i], (size_t)flen[(size_t)i] * sizeof(double));
    }
  });
  for (int i = 0; i < n; i++)
    if (cf[(size_t)i] == SF_PT) cf[(size_t)i] = F_PT;
}

// The right operand of the interpolations in matrix-matrix form, and beta_k = the sum of a_kl over the strong C
// neighbours l of k (stored order): row k of M is e_k for a C point, else the strong C entries of row k -- each divided
// by beta_k when `scaled` -- and nothing when beta_k = 0.  Columns: C points of m in fine order (f2c).
static void strong_c_operand(const HostCSR &D, const Strength &S, const std::vector<int> &m, const std::vector<int> &f2c,
                             int nc, bool scaled, std::vector<double> &beta, HostCSR &M) {
  const int n = D.nrows;
  beta.assign((size_t)n, 0.0);
  std::vector<int> mlen((size_t)n, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t k = b; k < e; k++) {
      if (m[(size_t)k] == C_PT) {
        mlen[(size_t)k] = 1;
        continue;
      }
      double bk = 0.0;
      int cnt = 0;
      for_each_strong_entry(D, S, k, [&](int64_t q, int l) {
        if (m[(size_t)l] == C_PT) {
          bk += D.a[(size_t)q];
          cnt++;
        }
      });
      beta[(size_t)k] = bk;
      mlen[(size_t)k] = bk != 0.0 ? cnt : 0;
    }
  });
  M.nrows = n;
  M.ncols = nc;
  M.ia.assign((size_t)n + 1, 0);
  for (int k = 0; k < n; k++) M.ia[(size_t)k + 1] = M.ia[(size_t)k] + mlen[(size_t)k];
  M.ja.resize((size_t)M.nnz());
  M.a.resize((size_t)M.nnz());
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t k = b; k < e; k++) {
      int64_t w = M.ia[(size_t)k];
      if (m[(size_t)k] == C_PT) {
        M.ja[(size_t)w] = f2c[(size_t)k];
        M.a[(size_t)w] = 1.0;
        continue;
      }
      if (!mlen[(size_t)k]) continue;
      for_each_strong_entry(D, S, k, [&](int64_t q, int l) {
        if (m[(size_t)l] == C_PT) {
          M.ja[(size_t)w] = f2c[(size_t)l];
          M.a[(size_t)w] = scaled ? D.a[(size_t)q] / beta[(size_t)k] : D.a[(size_t)q];
          w++;
        }
      });
    }
  });
}

// Extended interpolation E(A, S, m) of the two-stage interpolation ("Two-stage extended
// interpolation"), in matrix-matrix form: numerators N = Lo * M by host_spgemm, then w_ij = -n_ij / d_i, then the
// truncation.  rows (optional): build these rows only (the C1 rows of the second stage); columns: C points of m in
// fine order.  Every row is one thread's, every sum runs in stored order.
static void two_stage_ext_operands(const HostCSR &D, const Strength &S, const std::vector<int> &m,
                                   const std::vector<int> *rows, HostCSR &Lo, HostCSR &M, std::vector<double> &d,
                                   int &nc_out) {
  const int n = D.nrows;
  std::vector<int> f2c;
  const int nc = nc_out = coarse_numbering(m, f2c);
  std::vector<double> beta;
  strong_c_operand(D, S, m, f2c, nc, true, beta, M);
  // left operand: C row -> (i, 1) (the unit row comes out of the product as 1 * 1), F row -> its strong entries,
  // special F row -> nothing; d_i of the F rows
  const int nr = rows ? (int)rows->size() : n;
  Lo.nrows = nr;
  Lo.ncols = n;
  Lo.ia.assign((size_t)nr + 1, 0);
  for (int r = 0; r < nr; r++) {
    const int i = rows ? (*rows)[(size_t)r] : r;
    const int64_t len = m[(size_t)i] == C_PT ? 1 : m[(size_t)i] == F_PT ? S.ia[(size_t)i + 1] - S.ia[(size_t)i] : 0;
    Lo.ia[(size_t)r + 1] = Lo.ia[(size_t)r] + len;
  }
  Lo.ja.resize((size_t)Lo.nnz());
  Lo.a.resize((size_t)Lo.nnz());
  d.assign((size_t)nr, 0.0);
  parallel_for(nr, [&](int64_t b, int64_t e, int) {
    for (int64_t r = b; r < e; r++) {
      const int i = rows ? (*rows)[(size_t)r] : (int)r;
      int64_t w = Lo.ia[(size_t)r];
      if (m[(size_t)i] == C_PT) {
        Lo.ja[(size_t)w] = i;
        Lo.a[(size_t)w] = 1.0;
        continue;
      }
      if (m[(size_t)i] != F_PT) continue;
      double di = 0.0;
      for_each_entry_strong(D, S, i, [&](int64_t q, int j, bool strong) {
        if (strong) {
          Lo.ja[(size_t)w] = j;
          Lo.a[(size_t)w] = D.a[(size_t)q];
          w++;
          if (m[(size_t)j] != C_PT && beta[(size_t)j] == 0.0) di += D.a[(size_t)q];
        } else
          di += D.a[(size_t)q];  // the diagonal and the weak entries
      });
      d[(size_t)r] = di;
    }
  });
}

void two_stage_zero_denominator(int level, int row) {
  fail(4, "BoomerAMGSetup: two-stage extended interpolation (agg_interp_type 5) on level " + std::to_string(level) +
              ": row " + std::to_string(row) + " has a zero denominator d_i with a non-empty numerator");
}

// rows of N in place: F rows become w = -n / d, then every row is truncated; compacted into P.  Returns -1, or the
// smallest F row with d_i = 0 and a non-empty numerator (P is then not built)
static int two_stage_finish_rows(HostCSR &N, const std::vector<int> *rows, const std::vector<int> *m,
                                 const std::vector<double> *d, double trunc_factor, int pmax, HostCSR &P) {
  const int nr = N.nrows;
  std::vector<int> flen((size_t)nr, 0);
  std::atomic<int> bad{-1};
  parallel_for(nr, [&](int64_t b, int64_t e, int) {
    std::vector<char> keep;
    for (int64_t r = b; r < e; r++) {
      const int64_t s0 = N.ia[(size_t)r];
      int len = (int)(N.ia[(size_t)r + 1] - s0);
      if (len == 0) continue;
      if (m) {
        const int i = rows ? (*rows)[(size_t)r] : (int)r;
        if ((*m)[(size_t)i] == F_PT) {
          const double di = (*d)[(size_t)r];
          if (di == 0.0) {
            int seen = bad.load();
            while ((seen < 0 || i < seen) && !bad.compare_exchange_weak(seen, i)) {
            }
            continue;
          }
          for (int k = 0; k < len; k++) N.a[(size_t)(s0 + k)] = -N.a[(size_t)(s0 + k)] / di;
        }
      }
      if (trunc_factor > 0.0 || pmax > 0)
        len = truncate_row(len, N.ja.data() + s0, N.a.data() + s0, trunc_factor, pmax, keep);
      flen[(size_t)r] = len;
    }
  });
  if (bad.load() >= 0) return bad.load();
  P.nrows = nr;
  P.ncols = N.ncols;
  P.ia.assign((size_t)nr + 1, 0);
  for (int r = 0; r < nr; r++) P.ia[(size_t)r + 1] = P.ia[(size_t)r] + flen[(size_t)r];
  P.ja.resize((size_t)P.nnz());
  P.a.resize((size_t)P.nnz());
  parallel_for(nr, [&](int64_t b, int64_t e, int) {
    for (int64_t r = b; r < e; r++) {
      if (!flen[(size_t)r]) continue;
      memcpy(P.ja.data() + P.ia[(size_t)r], N.ja.data() + N.ia[(size_t)r], (size_t)flen[(size_t)r] * sizeof(int));
      memcpy(P.a.data() + P.ia[(size_t)r], N.a.data() + N.ia[(size_t)r], (size_t)flen[(size_t)r] * sizeof(double));
    }
  });
  return -1;
}

// Two-stage extended interpolation of an aggressive level (agg_interp_type 5; Yang 2010, in the matrix-matrix form of
// Li, Sjogreen, Yang 2021): P = P1 * P2 with P1 = E(A, S, m1) (n x |C1|) and P2 = the C1 rows of E(A, S, m2)
// (|C1| x |C2|); P1 and P2 truncated by the P12 parameters, P by the aggressive ones.  m2 is handed on as multipass
// hands it on (special F -> F).  Returns -1, or the row with a zero denominator (P is then not built).
int build_two_stage_ext(const ParCSR &A, const Strength &S, const std::vector<int> &m1, std::vector<int> &m2,
                        double p12_trunc_factor, int p12_max, double trunc_factor, int pmax, HostCSR &P, int &nc_out) {
  const HostCSR &D = A.diag;
  const int n = D.nrows;
  std::vector<int> c1;
  for (int i = 0; i < n; i++)
    if (m1[(size_t)i] == C_PT) c1.push_back(i);
  HostCSR Lo, M, N, P1, P2;
  std::vector<double> d;
  int nc1 = 0;
  two_stage_ext_operands(D, S, m1, nullptr, Lo, M, d, nc1);
  host_spgemm(Lo, M, N);
  int bad = two_stage_finish_rows(N, nullptr, &m1, &d, p12_trunc_factor, p12_max, P1);
  if (bad >= 0) return bad;
  two_stage_ext_operands(D, S, m2, &c1, Lo, M, d, nc_out);
  host_spgemm(Lo, M, N);
  bad = two_stage_finish_rows(N, &c1, &m2, &d, p12_trunc_factor, p12_max, P2);
  if (bad >= 0) return bad;
  host_spgemm(P1, P2, N);
  two_stage_finish_rows(N, nullptr, nullptr, nullptr, trunc_factor, pmax, P);
  for (int i = 0; i < n; i++)
    if (m2[(size_t)i] == SF_PT) m2[(size_t)i] = F_PT;
  return -1;
}

// Operands of the extended+i interpolation in matrix-matrix form (interp_type 17; DESIGN.md section 3, "Matrix-matrix
// extended interpolation"): left operand B (n x n) with d, right operand Ah (n x |C|).  F row i is walked once in stored
// order: the diagonal and the weak entries go to d_i, a strong C neighbour k gives b_ik = a_ik, a strong neighbour k
// that is not a C point gives b_ik = a_ik / (beta_k + a_ki) and adds b_ik * a_ki to d_i -- or adds a_ik to d_i when
// beta_k or beta_k + a_ki is zero.  Ah_k = e_k for a C point, the unscaled strong C entries of row k otherwise (none
// when beta_k = 0).  Every row is one thread's, every sum runs in stored order.
static void mm_extpi_operands(const HostCSR &D, const Strength &S, const std::vector<int> &m, HostCSR &B, HostCSR &Ah,
                              std::vector<double> &d, int &nc_out) {
  const int n = D.nrows;
  std::vector<int> f2c;
  const int nc = nc_out = coarse_numbering(m, f2c);
  std::vector<double> beta;
  strong_c_operand(D, S, m, f2c, nc, false, beta, Ah);
  // a_ki: the stored entry (k, i), or 0
  auto entry = [&](int k, int i) {
    const int *r0 = D.ja.data() + D.ia[(size_t)k], *r1 = D.ja.data() + D.ia[(size_t)k + 1];
    const int *it = std::lower_bound(r0, r1, i);
    return (it != r1 && *it == i) ? D.a[(size_t)(it - D.ja.data())] : 0.0;
  };
  // one walk of F row i: what(j, kind, b, term) -- kind 0: term goes to d_i; 1: (j, b) goes to B; 2: both
  auto walk = [&](int i, auto &&what) {
    for_each_entry_strong(D, S, i, [&](int64_t q, int j, bool strong) {
      const double v = D.a[(size_t)q];
      if (!strong) {
        what(j, 0, 0.0, v);  // the diagonal and the weak entries
      } else if (m[(size_t)j] == C_PT) {
        what(j, 1, v, 0.0);
      } else if (beta[(size_t)j] == 0.0) {
        what(j, 0, 0.0, v);
      } else {
        const double aki = entry(j, i);
        const double delta = beta[(size_t)j] + aki;
        if (delta == 0.0) {
          what(j, 0, 0.0, v);
        } else {
          const double bik = v / delta;
          const double prod = bik * aki;  // (one product, rounded on its own)
          what(j, 2, bik, prod);
        }
      }
    });
  };
  B.nrows = n;
  B.ncols = n;
  B.ia.assign((size_t)n + 1, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int c = 0;
      if (m[(size_t)i] == C_PT)
        c = 1;
      else if (m[(size_t)i] == F_PT)
        walk((int)i, [&](int, int kind, double, double) { c += kind != 0; });
      B.ia[(size_t)i + 1] = c;
    }
  });
  for (int i = 0; i < n; i++) B.ia[(size_t)i + 1] += B.ia[(size_t)i];
  B.ja.resize((size_t)B.nnz());
  B.a.resize((size_t)B.nnz());
  d.assign((size_t)n, 0.0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int64_t w = B.ia[(size_t)i];
      if (m[(size_t)i] == C_PT) {
        B.ja[(size_t)w] = (int)i;
        B.a[(size_t)w] = 1.0;
        continue;
      }
      if (m[(size_t)i] != F_PT) continue;
      double di = 0.0;
      walk((int)i, [&](int j, int kind, double bik, double term) {
        if (kind != 0) {
          B.ja[(size_t)w] = j;
          B.a[(size_t)w] = bik;
          w++;
        }
        if (kind != 1) di += term;
      });
      d[(size_t)i] = di;
    }
  });
}

void mm_interp_zero_denominator(int interp_type, int level, int row) {
  fail(4, "BoomerAMGSetup: matrix-matrix extended interpolation (interp_type " + std::to_string(interp_type) + ") on level " +
              std::to_string(level) + ": row " + std::to_string(row) +
              " has a zero denominator d_i with a non-empty numerator");
}

// Extended (16) and extended+i (17) interpolation in matrix-matrix form (Li, Sjogreen, Yang 2021):
// numerators N = B * Ah by host_spgemm, w_ij = -n_ij / d_i, truncation.  Type 16 is E(A, S, cf) of the two-stage
// interpolation on the level's own marker.  cf is handed on with special F -> F.  Returns -1, or the row with a zero
// denominator (P is then not built).
int build_mm_interp(const ParCSR &A, const Strength &S, std::vector<int> &cf, int interp_type, double trunc_factor,
                    int pmax, HostCSR &P, int &nc_out) {
  const HostCSR &D = A.diag;
  HostCSR B, Ah, N;
  std::vector<double> d;
  if (interp_type == 16)
    two_stage_ext_operands(D, S, cf, nullptr, B, Ah, d, nc_out);
  else
    mm_extpi_operands(D, S, cf, B, Ah, d, nc_out);
  host_spgemm(B, Ah, N);
  const int bad = two_stage_finish_rows(N, nullptr, &cf, &d, trunc_factor, pmax, P);
  if (bad >= 0) return bad;
  for (size_t i = 0; i < cf.size(); i++)
    if (cf[i] == SF_PT) cf[i] = F_PT;
  return -1;
}

void air_singular_system(int level, int row) {
  fail(4, "BoomerAMGSetup: approximate ideal restriction (restriction 1) on level " + std::to_string(level) + ": row " +
              std::to_string(row) + " has a singular local system A[N_i, N_i]; refusing to substitute another restriction");
}

// Distance-1 approximate ideal restriction (restriction 1; Manteuffel, Ruge, Southworth 2018; DESIGN.md section 3,
// "Approximate ideal restriction"), bit for bit sk::air_restriction but for neighbourhoods of any size.  For a C point i,
// N_i = the F columns j != i with |a_ij| >= theta_r * max_{k != i} |a_ik| (ascending); M[t][c] = a(N_c, N_t) and the
// right-hand side -a(i, N_t) are eliminated with partial pivoting -- the pivot of step k is the unused row with the
// largest |value| in column k, the lowest row on a tie; rows are not moved -- and substituted back by columns,
// descending.  Row c(i) of R = (N_t, y_t), less the entries with |y_t| < phi * max_s |y_s| (phi > 0), and (i, 1.0).
// Returns -1, or the smallest C row whose local system is singular (R is then not built).
int build_air_restriction(const HostCSR &D, const std::vector<int> &cf, double theta_r, double phi, HostCSR &R,
                          sk::AirInfo &info) {
  const int n = D.nrows;
  info = sk::AirInfo();
  std::vector<int> c2f;
  for (int i = 0; i < n; i++)
    if (cf[(size_t)i] == C_PT) c2f.push_back(i);
  const int nc = (int)c2f.size();
  auto neighbourhood = [&](int i, auto &&emit) {
    double mx = 0.0;
    for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++)
      if (D.ja[(size_t)k] != i) mx = std::fmax(mx, std::fabs(D.a[(size_t)k]));
    if (!(mx > 0.0)) return;
    const double thr = theta_r * mx;
    for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++) {
      const int j = D.ja[(size_t)k];
      if (j == i || cf[(size_t)j] == C_PT || !(std::fabs(D.a[(size_t)k]) >= thr)) continue;
      emit(j, D.a[(size_t)k]);
    }
  };
  // a_rc: the stored entry (r, c), or 0
  auto entry = [&](int r, int c) {
    const int *r0 = D.ja.data() + D.ia[(size_t)r], *r1 = D.ja.data() + D.ia[(size_t)r + 1];
    const int *it = std::lower_bound(r0, r1, c);
    return (it != r1 && *it == c) ? D.a[(size_t)(it - D.ja.data())] : 0.0;
  };
  // rows with slack (1 + |N_i| entries), compacted afterwards
  std::vector<int64_t> sia((size_t)nc + 1, 0);
  parallel_for(nc, [&](int64_t b, int64_t e, int) {
    for (int64_t c = b; c < e; c++) {
      int m = 0;
      neighbourhood(c2f[(size_t)c], [&](int, double) { m++; });
      sia[(size_t)c + 1] = m + 1;
    }
  });
  int max_m = 0, zero_rows = 0;
  for (int c = 0; c < nc; c++) {
    const int m = (int)sia[(size_t)c + 1] - 1;
    max_m = std::max(max_m, m);
    zero_rows += m == 0;
    sia[(size_t)c + 1] += sia[(size_t)c];
  }
  std::vector<int> sja((size_t)sia[(size_t)nc]);
  std::vector<double> sa((size_t)sia[(size_t)nc]);
  std::vector<int> len((size_t)nc, 0);
  std::atomic<int> bad{-1};
  parallel_for(nc, [&](int64_t b, int64_t e, int) {
    std::vector<int> N, piv, step;
    std::vector<double> M, y;
    std::vector<char> used;
    for (int64_t c = b; c < e; c++) {
      const int i = c2f[(size_t)c];
      N.clear();
      y.clear();
      neighbourhood(i, [&](int j, double v) {
        N.push_back(j);
        y.push_back(v);  // g_t, for now
      });
      const int m = (int)N.size(), ld = m + 1;
      M.assign((size_t)m * (size_t)ld, 0.0);
      for (int t = 0; t < m; t++) {
        for (int q = 0; q < m; q++) M[(size_t)t * ld + q] = entry(N[(size_t)q], N[(size_t)t]);
        M[(size_t)t * ld + m] = -y[(size_t)t];
      }
      used.assign((size_t)m, 0);
      step.assign((size_t)m, m);
      piv.assign((size_t)m, 0);
      bool singular = false;
      for (int k = 0; k < m && !singular; k++) {
        int idx = -1;
        double v = -1.0;
        for (int t = 0; t < m; t++)
          if (!used[(size_t)t] && std::fabs(M[(size_t)t * ld + k]) > v) v = std::fabs(M[(size_t)t * ld + k]), idx = t;
        if (!(v > 0.0)) {
          singular = true;
          break;
        }
        piv[(size_t)k] = idx;
        used[(size_t)idx] = 1;
        step[(size_t)idx] = k;
        const double *Mp = &M[(size_t)idx * ld];
        for (int t = 0; t < m; t++) {
          if (used[(size_t)t]) continue;
          double *Mt = &M[(size_t)t * ld];
          const double l = Mt[k] / Mp[k];
          for (int q = k + 1; q < m; q++) Mt[q] = Mt[q] - l * Mp[q];
          Mt[m] = Mt[m] - l * Mp[m];
        }
      }
      if (singular) {
        int cur = bad.load();
        while ((cur < 0 || i < cur) && !bad.compare_exchange_weak(cur, i)) {
        }
        continue;
      }
      for (int q = m - 1; q >= 0; q--) {
        const double *Mp = &M[(size_t)piv[(size_t)q] * ld];
        y[(size_t)q] = Mp[m] / Mp[q];
        for (int t = 0; t < m; t++)
          if (step[(size_t)t] < q) M[(size_t)t * ld + m] = M[(size_t)t * ld + m] - M[(size_t)t * ld + q] * y[(size_t)q];
      }
      double mx = 0.0;
      if (phi > 0.0)
        for (int t = 0; t < m; t++) mx = std::fmax(mx, std::fabs(y[(size_t)t]));
      const double thr = phi * mx;
      int64_t w = sia[(size_t)c];
      bool unit_done = false;
      for (int t = 0; t < m; t++) {
        if (phi > 0.0 && std::fabs(y[(size_t)t]) < thr) continue;
        if (!unit_done && N[(size_t)t] > i) sja[(size_t)w] = i, sa[(size_t)w] = 1.0, w++, unit_done = true;
        sja[(size_t)w] = N[(size_t)t], sa[(size_t)w] = y[(size_t)t], w++;
      }
      if (!unit_done) sja[(size_t)w] = i, sa[(size_t)w] = 1.0, w++;
      len[(size_t)c] = (int)(w - sia[(size_t)c]);
    }
  });
  info.max_m = max_m;
  info.zero_rows = zero_rows;
  if (bad.load() >= 0) {
    info.bad_row = bad.load();
    return bad.load();
  }
  R.nrows = nc;
  R.ncols = n;
  R.ia.assign((size_t)nc + 1, 0);
  for (int c = 0; c < nc; c++) R.ia[(size_t)c + 1] = R.ia[(size_t)c] + len[(size_t)c];
  R.ja.resize((size_t)R.nnz());
  R.a.resize((size_t)R.nnz());
  parallel_for(nc, [&](int64_t b, int64_t e, int) {
    for (int64_t c = b; c < e; c++) {
      memcpy(R.ja.data() + R.ia[(size_t)c], sja.data() + sia[(size_t)c], (size_t)len[(size_t)c] * sizeof(int));
      memcpy(R.a.data() + R.ia[(size_t)c], sa.data() + sia[(size_t)c], (size_t)len[(size_t)c] * sizeof(double));
    }
  });
  info.dropped = sia[(size_t)nc] - R.nnz();
  return -1;
}

// FSAI with the adaptive pattern (fsai_algo_type 4; DESIGN.md section 3, "FSAI (adaptive pattern)"), bit for bit
// sk::fsai_adaptive.  Row i starts from P = (i); a step solves B[P, P]^T y = e_last (the elimination of the static
// path: partial pivoting, the lowest row on a tie, rows not moved, back substitution by columns, descending), tests
// psi = 1 / y_last against the previous one, sums phi_j = sum_{r in P ascending, i last} b_rj y_r over the stored columns
// j < i outside P -- one `acc = acc + b * y` per entry, from 0.0 --, and moves the up to T columns with the largest
// |phi_j| > 0 (the lower column on a tie) into P.  Row i of G = y / sqrt(y_last) on P.  Returns 0, or 2 when a row
// fails (info.bad_row = the smallest such row; G is not built).
int build_fsai_adaptive(const HostCSR &B, int S, int T, double tau, HostCSR &G, sk::FsaiAdaptiveInfo &info) {
  const int n = B.nrows;
  info = sk::FsaiAdaptiveInfo();
  struct Part {
    int64_t b = 0;
    std::vector<int> ja;
    std::vector<double> a;
  };
  std::vector<Part> parts;
  std::vector<int> len((size_t)n, 0);
  std::mutex mu;
  auto entry = [&](int r, int c) {
    const int *r0 = B.ja.data() + B.ia[(size_t)r], *r1 = B.ja.data() + B.ia[(size_t)r + 1];
    const int *it = std::lower_bound(r0, r1, c);
    return (it != r1 && *it == c) ? B.a[(size_t)(it - B.ja.data())] : 0.0;
  };
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    Part part;
    part.b = b;
    sk::FsaiAdaptiveInfo loc;
    std::vector<int> pos((size_t)n, -1);  // column -> its candidate; -2: in the pattern
    std::vector<int> P, cj, piv, step, chosen;
    std::vector<double> M, y, cv;
    std::vector<char> used, taken;
    for (int64_t i64 = b; i64 < e; i64++) {
      const int i = (int)i64;
      P.assign(1, i);
      int stop = 0, failed = 0;
      double psi = 0.0;
      for (int st = 0; st <= S && !stop; st++) {
        const int m = (int)P.size(), ld = m + 1;
        M.assign((size_t)m * (size_t)ld, 0.0);
        for (int t = 0; t < m; t++) {
          for (int q = 0; q < m; q++) M[(size_t)t * ld + q] = entry(P[(size_t)q], P[(size_t)t]);
          M[(size_t)t * ld + m] = (t == m - 1) ? 1.0 : 0.0;
        }
        used.assign((size_t)m, 0);
        step.assign((size_t)m, m);
        piv.assign((size_t)m, 0);
        for (int k = 0; k < m && !failed; k++) {
          int idx = -1;
          double v = -1.0;
          for (int t = 0; t < m; t++)
            if (!used[(size_t)t] && std::fabs(M[(size_t)t * ld + k]) > v) v = std::fabs(M[(size_t)t * ld + k]), idx = t;
          if (!(v > 0.0)) {
            failed = 1;
            break;
          }
          piv[(size_t)k] = idx;
          used[(size_t)idx] = 1;
          step[(size_t)idx] = k;
          const double *Mp = &M[(size_t)idx * ld];
          for (int t = 0; t < m; t++) {
            if (used[(size_t)t]) continue;
            double *Mt = &M[(size_t)t * ld];
            const double l = Mt[k] / Mp[k];
            for (int q = k + 1; q < m; q++) Mt[q] = Mt[q] - l * Mp[q];
            Mt[m] = Mt[m] - l * Mp[m];
          }
        }
        if (failed) break;
        y.assign((size_t)m, 0.0);
        for (int q = m - 1; q >= 0; q--) {
          const double *Mp = &M[(size_t)piv[(size_t)q] * ld];
          y[(size_t)q] = Mp[m] / Mp[q];
          for (int t = 0; t < m; t++)
            if (step[(size_t)t] < q) M[(size_t)t * ld + m] = M[(size_t)t * ld + m] - M[(size_t)t * ld + q] * y[(size_t)q];
        }
        const double ylast = y[(size_t)m - 1];
        if (!(ylast > 0.0)) {
          failed = 2;
          break;
        }
        const double psin = 1.0 / ylast;
        if (st > 0 && psi - psin < tau * psi)
          stop = 1;
        else if (st == S)
          stop = 3;
        else
          psi = psin;
        if (stop) break;
        // the gradient on the stored columns j < i outside P
        cj.clear();
        cv.clear();
        for (int q = 0; q < m; q++) pos[(size_t)P[(size_t)q]] = -2;
        for (int q = 0; q < m; q++) {
          const int r = P[(size_t)q];
          for (int64_t k = B.ia[(size_t)r]; k < B.ia[(size_t)r + 1]; k++) {
            const int j = B.ja[(size_t)k];
            if (j >= i) break;
            int &pj = pos[(size_t)j];
            if (pj == -2) continue;
            if (pj < 0) {
              pj = (int)cj.size();
              cj.push_back(j);
              cv.push_back(0.0);
            }
            cv[(size_t)pj] = cv[(size_t)pj] + B.a[(size_t)k] * y[(size_t)q];
          }
        }
        int nc = 0;
        for (double v : cv) nc += std::fabs(v) > 0.0;
        loc.max_candidates = std::max(loc.max_candidates, nc);
        taken.assign(cj.size(), 0);
        chosen.clear();
        for (int round = 0; round < T; round++) {
          double bv = -1.0;
          int bj = INT_MAX, bs = -1;
          for (size_t u = 0; u < cj.size(); u++) {
            const double v = std::fabs(cv[u]);
            if (taken[u] || !(v > 0.0)) continue;
            if (v > bv || (v == bv && cj[u] < bj)) bv = v, bj = cj[u], bs = (int)u;
          }
          if (bs < 0) break;
          taken[(size_t)bs] = 1;
          chosen.push_back(bj);
        }
        for (int j : cj) pos[(size_t)j] = -1;
        for (int q = 0; q < m; q++) pos[(size_t)P[(size_t)q]] = -1;
        if (chosen.empty()) {
          stop = 2;
          break;
        }
        P.pop_back();
        P.insert(P.end(), chosen.begin(), chosen.end());
        std::sort(P.begin(), P.end());
        P.push_back(i);
      }
      if (failed) {
        std::lock_guard<std::mutex> lock(mu);
        if (info.bad_row < 0 || i < info.bad_row) info.bad_row = i, info.bad_kind = failed;
        continue;
      }
      const int m = (int)P.size();
      const double d = std::sqrt(y[(size_t)m - 1]);
      for (int q = 0; q < m; q++) {
        part.ja.push_back(P[(size_t)q]);
        part.a.push_back(y[(size_t)q] / d);
      }
      len[(size_t)i] = m;
      loc.max_row = std::max(loc.max_row, m);
      (stop == 1 ? loc.stop_tolerance : (stop == 2 ? loc.stop_no_candidate : loc.stop_max_steps))++;
    }
    std::lock_guard<std::mutex> lock(mu);
    info.max_row = std::max(info.max_row, loc.max_row);
    info.max_candidates = std::max(info.max_candidates, loc.max_candidates);
    info.stop_tolerance += loc.stop_tolerance;
    info.stop_no_candidate += loc.stop_no_candidate;
    info.stop_max_steps += loc.stop_max_steps;
    parts.push_back(std::move(part));
  });
  if (info.bad_row >= 0) {
    info.status = 2;
    return 2;
  }
  G.nrows = n;
  G.ncols = B.ncols;
  G.ia.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) G.ia[(size_t)i + 1] = G.ia[(size_t)i] + len[(size_t)i];
  G.ja.resize((size_t)G.nnz());
  G.a.resize((size_t)G.nnz());
  for (const Part &part : parts) {
    if (part.ja.empty()) continue;
    memcpy(G.ja.data() + G.ia[(size_t)part.b], part.ja.data(), part.ja.size() * sizeof(int));
    memcpy(G.a.data() + G.ia[(size_t)part.b], part.a.data(), part.a.size() * sizeof(double));
  }
  return 0;
}

// One-point interpolation (interp_type 100), bit for bit sk::one_point_interp: a C point i gets
// (c(i), 1.0); an F point i the C point j of its row of S with the largest |a_ij|, the lowest column on a tie, as
// (c(j), 1.0) -- or an empty row.  Truncation does not apply.  cf is handed on with special F -> F.
void build_one_point_interp(const HostCSR &D, const Strength &S, std::vector<int> &cf, HostCSR &P, int &nc_out) {
  const int n = D.nrows;
  std::vector<int> f2c, sel((size_t)n, -1);
  const int nc = nc_out = coarse_numbering(cf, f2c);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      if (cf[(size_t)i] == C_PT) {
        sel[(size_t)i] = f2c[(size_t)i];
        continue;
      }
      double best = -1.0;
      for_each_strong_entry(D, S, i, [&](int64_t k, int j) {
        if (cf[(size_t)j] == C_PT && std::fabs(D.a[(size_t)k]) > best)
          best = std::fabs(D.a[(size_t)k]), sel[(size_t)i] = f2c[(size_t)j];
      });
    }
  });
  P.nrows = n;
  P.ncols = nc;
  P.ia.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) P.ia[(size_t)i + 1] = P.ia[(size_t)i] + (sel[(size_t)i] >= 0);
  P.ja.resize((size_t)P.nnz());
  P.a.assign((size_t)P.nnz(), 1.0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++)
      if (sel[(size_t)i] >= 0) P.ja[(size_t)P.ia[(size_t)i]] = sel[(size_t)i];
  });
  for (size_t i = 0; i < cf.size(); i++)
    if (cf[i] == SF_PT) cf[i] = F_PT;
}

void dense_inverse(int n, std::vector<double> &M, std::vector<double> &inv) {
  inv.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) inv[(size_t)i * n + i] = 1.0;
  for (int c = 0; c < n; c++) {
    int piv = c;
    for (int r = c + 1; r < n; r++)
      if (std::fabs(M[(size_t)r * n + c]) > std::fabs(M[(size_t)piv * n + c])) piv = r;
    if (piv != c)
      for (int j = 0; j < n; j++) {
        std::swap(M[(size_t)c * n + j], M[(size_t)piv * n + j]);
        std::swap(inv[(size_t)c * n + j], inv[(size_t)piv * n + j]);
      }
    const double d = M[(size_t)c * n + c];
    if (d == 0.0) continue;
    const double id = 1.0 / d;
    for (int j = 0; j < n; j++) {
      M[(size_t)c * n + j] *= id;
      inv[(size_t)c * n + j] *= id;
    }
    for (int r = 0; r < n; r++) {
      if (r == c) continue;
      const double f = M[(size_t)r * n + c];
      if (f == 0.0) continue;
      for (int j = 0; j < n; j++) {
        M[(size_t)r * n + j] -= f * M[(size_t)c * n + j];
        inv[(size_t)r * n + j] -= f * inv[(size_t)c * n + j];
      }
    }
  }
}

// l1 norms; chunk = hybrid-GS chunk ("thread") size; cf_ext = C/F type of the halo columns
void level_norms(const ParCSR &A, const std::vector<int> &cf, const std::vector<int> &cf_ext, int chunk,
                 std::vector<double> &diag, std::vector<double> &l1gs, std::vector<double> &l1jac) {
  const HostCSR &D = A.diag, &O = A.offd;
  const int n = D.nrows;
  diag.assign((size_t)n, 0.0);
  l1gs.assign((size_t)n, 0.0);
  l1jac.assign((size_t)n, 0.0);
  const bool has_cf = !cf.empty();
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      const int64_t cs = (i / chunk) * chunk, ce = cs + chunk;
      double d = 0.0, l1 = 0.0, full = 0.0;
      for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++) {
        const int j = D.ja[(size_t)k];
        const double av = std::fabs(D.a[(size_t)k]);
        full += av;
        if (j == i) {
          d = D.a[(size_t)k];
          l1 += av;
        } else if (j < cs || j >= ce) {
          if (!has_cf || cf[(size_t)j] == cf[(size_t)i]) l1 += 0.5 * av;
        }
      }
      for (int64_t k = O.ia[(size_t)i]; k < O.ia[(size_t)i + 1]; k++) {
        const double av = std::fabs(O.a[(size_t)k]);
        full += av;
        if (!has_cf || cf_ext[(size_t)O.ja[(size_t)k]] == cf[(size_t)i]) l1 += 0.5 * av;
      }
      if (l1 <= 4.0 / 3.0 * std::fabs(d)) l1 = std::fabs(d);
      if (d < 0) {
        l1 = -l1;
        full = -full;
      }
      diag[(size_t)i] = d;
      l1gs[(size_t)i] = l1;
      l1jac[(size_t)i] = full;
    }
  });
}

}  // namespace hs
using namespace hs;

void host_transpose(const HostCSR &A, HostCSR &T) {
  T.nrows = A.ncols;
  T.ncols = A.nrows;
  T.ia.assign((size_t)A.ncols + 1, 0);
  const int64_t nnz = A.nnz();
  for (int64_t k = 0; k < nnz; k++) T.ia[(size_t)A.ja[(size_t)k] + 1]++;
  for (int i = 0; i < A.ncols; i++) T.ia[(size_t)i + 1] += T.ia[(size_t)i];
  T.ja.resize((size_t)nnz);
  T.a.resize((size_t)nnz);
  std::vector<int64_t> pos(T.ia.begin(), T.ia.end() - 1);
  for (int i = 0; i < A.nrows; i++)
    for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) {
      const int64_t q = pos[(size_t)A.ja[(size_t)k]]++;
      T.ja[(size_t)q] = i;
      T.a[(size_t)q] = A.a[(size_t)k];
    }
}

// Gustavson row products with a dense accumulator per thread; the accumulation
// order inside a row is (k ascending in A's row) x (stored order of B's row k),
// output columns ascending
void host_spgemm(const HostCSR &A, const HostCSR &B, HostCSR &C) {
  const int n = A.nrows, m = B.ncols;
  C.nrows = n;
  C.ncols = m;
  C.ia.assign((size_t)n + 1, 0);
  std::vector<int> cnt((size_t)n, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    std::vector<int> mark((size_t)m, -1);
    for (int64_t i = b; i < e; i++) {
      int c = 0;
      for (int64_t ka = A.ia[(size_t)i]; ka < A.ia[(size_t)i + 1]; ka++) {
        const int kr = A.ja[(size_t)ka];
        for (int64_t kb = B.ia[(size_t)kr]; kb < B.ia[(size_t)kr + 1]; kb++) {
          const int j = B.ja[(size_t)kb];
          if (mark[(size_t)j] != i) {
            mark[(size_t)j] = (int)i;
            c++;
          }
        }
      }
      cnt[(size_t)i] = c;
    }
  }, 16);
  for (int i = 0; i < n; i++) C.ia[(size_t)i + 1] = C.ia[(size_t)i] + cnt[(size_t)i];
  C.ja.resize((size_t)C.nnz());
  C.a.resize((size_t)C.nnz());
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    std::vector<int> mark((size_t)m, -1);
    std::vector<double> acc((size_t)m, 0.0);
    for (int64_t i = b; i < e; i++) {
      int64_t q = C.ia[(size_t)i];
      for (int64_t ka = A.ia[(size_t)i]; ka < A.ia[(size_t)i + 1]; ka++) {
        const int kr = A.ja[(size_t)ka];
        const double av = A.a[(size_t)ka];
        for (int64_t kb = B.ia[(size_t)kr]; kb < B.ia[(size_t)kr + 1]; kb++) {
          const int j = B.ja[(size_t)kb];
          if (mark[(size_t)j] != i) {
            mark[(size_t)j] = (int)i;
            C.ja[(size_t)q++] = j;
            acc[(size_t)j] = av * B.a[(size_t)kb];
          } else
            acc[(size_t)j] += av * B.a[(size_t)kb];
        }
      }
      std::sort(C.ja.begin() + C.ia[(size_t)i], C.ja.begin() + C.ia[(size_t)i + 1]);
      for (int64_t k = C.ia[(size_t)i]; k < C.ia[(size_t)i + 1]; k++) C.a[(size_t)k] = acc[(size_t)C.ja[(size_t)k]];
    }
  }, 16);
}

long long BoomerAMG::default_device_min_rows() {
  const char *e = getenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS");
  return e ? atoll(e) : 20000;
}

void BoomerAMG::use_private_self_comm() {
  own_comm = make_self_comm();
  forced_comm = own_comm.get();
}

long long BoomerAMG::effective_redundant_rows() const {
  if (p.redundant_rows >= 0) return p.redundant_rows;
  const char *e = getenv("MI_HYPRE_REDUNDANT_ROWS");
  return e ? atoll(e) : 200000;
}

void BoomerAMG::ensure_host(int level) {
  if (level < 0 || level >= (int)L.size()) return;
  AmgLevel &Lv = L[(size_t)level];
  fetch_operator(Lv.A, Lv.oA);
  fetch_operator(Lv.Pm.get(), Lv.oP);
  fetch_operator(Lv.Rm.get(), Lv.oR);
}

int BoomerAMG::chunk() const { return p.gs_chunk > 0 ? p.gs_chunk : ctx().gs_chunk; }

// Sum of the levels' entries over the entries of level 0.  On N > 1 ranks the GLOBAL figure (what HYPRE prints), summed
// over the ranks once at the end of Setup, where every rank is present -- the getter itself is not collective.
double BoomerAMG::operator_complexity() const {
  if (L.empty()) return 0.0;
  if (global_opcx >= 0.0) return global_opcx;
  double num = 0.0, den = 0.0;
  local_entry_counts(num, den);
  return den > 0 ? num / den : 0.0;
}

void BoomerAMG::local_entry_counts(double &tot_out, double &base_out) const {
  double tot = 0.0;
  const size_t own = tail ? L.size() - 1 : L.size();  // the stub's operator is the tail's fine level
  for (size_t l = 0; l < own; l++) tot += (double)(L[l].A->diag_nnz() + L[l].A->offd.nnz());
  if (tail) {
    double t = 0.0;
    for (const auto &l : tail->L) t += (double)(l.A->diag_nnz() + l.A->offd.nnz());
    tot += t / (double)std::max(1, my_comm().size);  // this rank's share of the redundant levels
  }
  tot_out = tot;
  base_out = (double)(L[0].A->diag_nnz() + L[0].A->offd.nnz());
}

// C-first ordering.  The hierarchy above is built in natural
// order; here every level with a C/F splitting is renumbered inside its rank:
// C points first (original order kept, so C point q IS coarse unknown q of the
// rank), F points after.  Chunks of 8 rows are then all-C or all-F (bar one
// mixed chunk per rank), a C or F relaxation pass touches one contiguous row
// range, and the two passes of a sweep stream the level's matrix once instead of
// twice.  Halo columns are renumbered by their owners (one halo exchange of the
// new positions), so the level gets a fresh col_map_offd and halo plan.  Level 0
// becomes a renumbered COPY of the caller's matrix, which stays untouched.
void BoomerAMG::apply_cf_ordering() {
  Comm &comm = my_comm();
  const size_t nlev = L.size();
  const bool timing = getenv("MI_HYPRE_SETUP_TIMING") != nullptr && comm.rank == 0;
  double tcf0 = wall_time();
  std::unique_ptr<TraceRange> trace_pos(new TraceRange("C-first: positions"));
  // old -> new local row, per level: on the device for the levels whose C/F marks live there (LazyInts: the levels
  // the device built), on the host for the others; hpos() / dpos() hand out the other side's copy when somebody needs it
  std::vector<std::vector<int>> pos(nlev);
  std::vector<DVec<int>> posd(nlev);
  std::vector<char> has_pos(nlev, 0);
  auto hpos = [&](size_t l) -> const std::vector<int> & {
    if (pos[l].empty() && posd[l].p && posd[l].n) pos[l] = posd[l].to_host();
    return pos[l];
  };
  auto dpos = [&](size_t l) -> const int * {
    if (!posd[l].p && !pos[l].empty()) posd[l].upload(pos[l]);
    return posd[l].p;
  };
  for (size_t l = 0; l < nlev; l++) {
    AmgLevel &Lv = L[l];
    if (Lv.cf.empty()) continue;
    const int n = Lv.A->nrows;
    has_pos[l] = 1;
    if (Lv.cf.on_device()) {
      hipStream_t s = ctx().stream;
      DVec<long long> crank;
      const long long nc_tot = sk::count_c_points(Lv.cf.dev(), n, crank, s);
      DVec<int> dperm((size_t)n);
      posd[l].alloc((size_t)n);
      sk::cfirst_order(Lv.cf.dev(), crank.p, n, (int)nc_tot, posd[l].p, dperm.p, s);
      Lv.nc = (int)nc_tot;
      Lv.perm.adopt_device(std::move(dperm), (size_t)n);
      continue;
    }
    const std::vector<int> &cfh = Lv.cf.host();
    pos[l].resize((size_t)n);
    std::vector<int> &permh = Lv.perm.hostw();
    permh.resize((size_t)n);
    // C points first, F points after, original order kept in both: the static partition of parallel_for is the
    // same in both passes (same n), so per-thread C counts give every thread its offsets
    const int nt = host_threads();
    std::vector<int64_t> cb((size_t)nt + 1, 0), ce((size_t)nt + 1, 0), ncnt((size_t)nt + 1, 0);
    parallel_for(n, [&](int64_t b, int64_t e, int t) {
      int64_t c = 0;
      for (int64_t i = b; i < e; i++) c += (cfh[(size_t)i] == C_PT);
      cb[(size_t)t] = b, ce[(size_t)t] = e, ncnt[(size_t)t] = c;
    });
    int64_t nc_tot = 0;
    for (int t = 0; t < nt; t++) nc_tot += ncnt[(size_t)t];
    Lv.nc = (int)nc_tot;
    std::vector<int64_t> coff((size_t)nt + 1, 0), foff((size_t)nt + 1, 0);
    {
      int64_t c = 0, f = nc_tot;
      for (int t = 0; t < nt; t++) {
        coff[(size_t)t] = c, foff[(size_t)t] = f;
        c += ncnt[(size_t)t];
        f += (ce[(size_t)t] - cb[(size_t)t]) - ncnt[(size_t)t];
      }
    }
    parallel_for(n, [&](int64_t b, int64_t e, int t) {
      int64_t c = coff[(size_t)t], f = foff[(size_t)t];
      for (int64_t i = b; i < e; i++) {
        const int q = (int)((cfh[(size_t)i] == C_PT) ? c++ : f++);
        pos[l][(size_t)i] = q;
        permh[(size_t)q] = (int)i;
      }
    });
  }
  // Relax types 40 / 41 / 42 (multicolour Gauss-Seidel): every level that is smoothed is coloured
  // -- the graph of D + D^T, D the level operator in the C-first numbering found above -- and the rows of its C block
  // and of its F block are sorted stably by colour; perm and the positions become those of the composed ordering, so
  // everything below (A, P, R, the marker, dof_func, the coarse numbering through P's columns) follows it.  A level
  // without a splitting (the coarsest) is one block.  The colouring and the sort run on the device, also for a level
  // the host routines built (its operator is uploaded for it).
  if (wants_mcgs()) {
    MI_REQUIRE(comm.size == 1, "multicolour Gauss-Seidel: one rank only");
    double t_colour = 0.0, t_sort = 0.0;
    for (size_t l = 0; l < nlev; l++) {
      AmgLevel &Lv = L[l];
      Lv.mc = AmgLevel::Colours();
      const int n = Lv.A->nrows;
      // the coarsest level when relax type 9 will solve it densely (build_coarsest_inverse) is not smoothed
      if (l + 1 == nlev && !tail && p.relax_type[2] == 9 && Lv.A->global_rows() <= MAX_DENSE && n > 0) continue;
      hipStream_t s = ctx().stream;
      double t0 = wall_time();
      sk::DCsr uploaded, cfirst;
      const sk::DCsr *D = &Lv.sA;
      if (!(Lv.sA.nrows == n && Lv.sA.ia.p)) {
        fetch_operator(Lv.A, Lv.sA);  // (an operator only the solve format holds, e.g. the caller's device-assembled matrix)
        uploaded.upload(Lv.A->diag, s);
        D = &uploaded;
      }
      if (has_pos[l]) {
        sk::permute(*D, Lv.perm.dev(), dpos(l), cfirst, s);
        D = &cfirst;
      }
      int kind = 0;
      const long long bad = sk::mcgs_bad_diagonal(*D, kind, s);
      if (bad >= 0) {
        long long row = has_pos[l] ? (long long)Lv.perm.host()[(size_t)bad] : bad;
        if (l == 0 && !input_order.empty()) row = input_order.host()[(size_t)row];
        fail(1, "BoomerAMGSetup: relax_type 40 / 41 / 42 (multicolour Gauss-Seidel): level " + std::to_string(l) + ", row " +
                    std::to_string(row) + " (the level's numbering before its ordering; level 0: the caller's local row) " +
                    (kind == 0 ? "stores no diagonal entry" : "stores a zero diagonal entry") +
                    "; refusing to smooth with something else");
      }
      DVec<int> colour;
      int rounds = 0;
      if (sk::ilu_multicolour(*D, colour, rounds, s) != 0)  // (no input reaches this: see IluSolver::multicolour_order)
        fail(1, "BoomerAMGSetup: the multicolour ordering of level " + std::to_string(l) + " left rows uncoloured after " +
                    std::to_string(n) + " rounds, one per row");
      MI_HIP(hipStreamSynchronize(s));
      t_colour += wall_time() - t0;
      t0 = wall_time();
      DVec<int> order;
      sk::mcgs_order(colour.p, n, has_pos[l] ? Lv.nc : 0, order, Lv.mc.range_start, Lv.mc.range_colour, Lv.mc.colours,
                     Lv.mc.ranges_c, s);
      Lv.mc.rounds = rounds;
      if (has_pos[l]) {  // stored row q is C-first row order[q], the level's row perm[order[q]]
        DVec<int> composed((size_t)n);
        sk::gather_elems(Lv.perm.dev(), order.p, 0, n, 4, composed.p, s);
        order = std::move(composed);
      } else {
        Lv.nc = 0;
      }
      pos[l].clear();
      posd[l].alloc((size_t)n);
      sk::invert_permutation(order.p, n, posd[l].p, s);
      MI_HIP(hipStreamSynchronize(s));
      Lv.perm.adopt_device(std::move(order), (size_t)n);
      has_pos[l] = 1;
      Lv.mc.ready = true;
      t_sort += wall_time() - t0;
      if (timing)
        printf("   multicolour ordering: level %zu: n %d, %d colours in %d rounds, %d + %d (block, colour) ranges\n", l, n,
               Lv.mc.colours, rounds, Lv.mc.ranges_c, (int)Lv.mc.range_colour.size() - Lv.mc.ranges_c);
    }
    if (timing) printf("   multicolour ordering: colouring %.3f s, sort %.3f s\n", t_colour, t_sort);
  }
  trace_pos.reset();
  if (timing) printf("   C-first ordering: positions %.2f s\n", wall_time() - tcf0);
  auto sort_rows = [](HostCSR &M) {
    parallel_for(M.nrows, [&](int64_t b, int64_t e, int) {
      std::vector<std::pair<int, double>> row;
      for (int64_t i = b; i < e; i++) {
        const int64_t s = M.ia[(size_t)i], len = M.ia[(size_t)i + 1] - s;
        bool sorted = true;
        for (int64_t k = 1; k < len; k++)
          if (M.ja[(size_t)(s + k)] < M.ja[(size_t)(s + k - 1)]) {
            sorted = false;
            break;
          }
        if (sorted) continue;
        row.resize((size_t)len);
        for (int64_t k = 0; k < len; k++) row[(size_t)k] = {M.ja[(size_t)(s + k)], M.a[(size_t)(s + k)]};
        std::sort(row.begin(), row.end(), [](const std::pair<int, double> &x, const std::pair<int, double> &y) {
          return x.first < y.first;
        });
        for (int64_t k = 0; k < len; k++) {
          M.ja[(size_t)(s + k)] = row[(size_t)k].first;
          M.a[(size_t)(s + k)] = row[(size_t)k].second;
        }
      }
    });
  };
  // B = rows of M taken in perm order, columns mapped through colpos (may be null)
  auto permute = [&](const HostCSR &M, const std::vector<int> &perm, const int *colpos, HostCSR &B) {
    const int n = M.nrows;
    B.nrows = n;
    B.ncols = M.ncols;
    B.ia.assign((size_t)n + 1, 0);
    for (int q = 0; q < n; q++) {
      const int i = perm.empty() ? q : perm[(size_t)q];
      B.ia[(size_t)q + 1] = B.ia[(size_t)q] + (M.ia[(size_t)i + 1] - M.ia[(size_t)i]);
    }
    B.ja.resize((size_t)B.nnz());
    B.a.resize((size_t)B.nnz());
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      for (int64_t q = b; q < e; q++) {
        const int i = perm.empty() ? (int)q : perm[(size_t)q];
        int64_t w = B.ia[(size_t)q];
        for (int64_t k = M.ia[(size_t)i]; k < M.ia[(size_t)i + 1]; k++, w++) {
          B.ja[(size_t)w] = colpos ? colpos[M.ja[(size_t)k]] : M.ja[(size_t)k];
          B.a[(size_t)w] = M.a[(size_t)k];
        }
      }
    });
    sort_rows(B);
  };
  for (size_t l = 0; l < nlev; l++) {
    AmgLevel &Lv = L[l];
    const double tl0 = wall_time();
    struct LevelTimer {
      bool on;
      size_t l;
      double t0;
      ~LevelTimer() {
        if (on) printf("   C-first ordering: level %zu %.2f s\n", l, wall_time() - t0);
      }
    } level_timer{timing && l < 4, l, tl0};
    TraceRange trace_lv(("C-first: level " + std::to_string(l)).c_str());
    // a level without C/F splitting (the coarsest) keeps its ordering: fetch it before sA goes away
    if (!has_pos[l] && Lv.sA.nrows == Lv.A->nrows) fetch_operator(Lv.A, Lv.sA);
    if (has_pos[l]) {
      ParCSR &A = *Lv.A;
      std::unique_ptr<ParCSR> An(new ParCSR());
      An->nrows = A.nrows;
      An->row_start = A.row_start;
      An->row_end = A.row_end;
      An->row_starts = A.row_starts;
      if (Lv.sA.nnz > 0 && Lv.sA.nrows == A.nrows) {
        hipStream_t s = ctx().stream;
        sk::permute(Lv.sA, Lv.perm.dev(), dpos(l), Lv.oA, s);
        An->diag.nrows = An->diag.ncols = A.nrows;
        An->host_diag_stale = true;
        An->dev_diag_nnz = Lv.oA.nnz;
      } else {
        if (A.host_diag_stale) fail(1, "C-first ordering: a level has neither host nor device arrays");
        permute(A.diag, Lv.perm.host(), hpos(l).data(), An->diag);
      }
      Lv.sA.release();
      // halo columns: new global id = owner's start + owner's new position
      const size_t next = A.col_map_offd.size();
      std::vector<int> ext_pos;
      if (comm.size > 1 || next > 0) ext_pos = A.halo_exchange_host_int(comm, hpos(l));
      std::vector<gidx> newgid(next);
      for (size_t k = 0; k < next; k++) {
        const gidx g = A.col_map_offd[k];
        const size_t owner =
            (size_t)(std::upper_bound(A.row_starts.begin(), A.row_starts.end(), g) - A.row_starts.begin()) - 1;
        newgid[k] = A.row_starts[owner] + ext_pos[k];
      }
      std::vector<gidx> cm(newgid);
      std::sort(cm.begin(), cm.end());
      std::vector<int> colpos(next);
      for (size_t k = 0; k < next; k++)
        colpos[k] = (int)(std::lower_bound(cm.begin(), cm.end(), newgid[k]) - cm.begin());
      if (A.offd.nnz() == 0) {  // no halo block (one rank): nothing to permute -- not even the row pointers
        An->offd.nrows = A.nrows;
        if (!An->host_diag_stale) An->offd.ia.assign((size_t)A.nrows + 1, 0);  // (device-resident: ParCSR::ensure_offd_rows)
      } else {
        permute(A.offd, Lv.perm.host(), next ? colpos.data() : nullptr, An->offd);
      }
      An->offd.ncols = (int)next;
      An->col_map_offd = cm;
      An->build_halo_plan(comm);
      Lv.A_own = std::move(An);
      Lv.A = Lv.A_own.get();
      if (Lv.cf.on_device() && Lv.perm.on_device()) {
        const size_t n = Lv.cf.size();
        DVec<int> cf2(n);
        sk::gather_elems(Lv.cf.dev(), Lv.perm.dev(), 0, (int)n, 4, cf2.p, ctx().stream);
        MI_HIP(hipStreamSynchronize(ctx().stream));
        Lv.cf.adopt_device(std::move(cf2), n);
      } else {
        const std::vector<int> &cfh = Lv.cf.host(), &permh = Lv.perm.host();
        std::vector<int> cf2(cfh.size());
        parallel_for((int64_t)cf2.size(), [&](int64_t b, int64_t e, int) {
          for (int64_t q = b; q < e; q++) cf2[(size_t)q] = cfh[(size_t)permh[(size_t)q]];
        });
        Lv.cf = std::move(cf2);
      }
      if (!Lv.dof.empty() && Lv.dof.on_device() && Lv.perm.on_device()) {  // (num_functions > 1) dof_func follows the rows
        const size_t n = Lv.dof.size();
        DVec<int> d2(n);
        sk::gather_elems(Lv.dof.dev(), Lv.perm.dev(), 0, (int)n, 4, d2.p, ctx().stream);
        MI_HIP(hipStreamSynchronize(ctx().stream));
        Lv.dof.adopt_device(std::move(d2), n);
      } else if (!Lv.dof.empty()) {
        const std::vector<int> &dh = Lv.dof.host(), &permh = Lv.perm.host();
        std::vector<int> d2(dh.size());
        for (size_t q = 0; q < d2.size(); q++) d2[q] = dh[(size_t)permh[q]];
        Lv.dof = std::move(d2);
      }
    }
    if (Lv.P.nrows > 0 && (has_pos[l] || (l + 1 < nlev && has_pos[l + 1]))) {
      const bool map_cols = l + 1 < nlev && has_pos[l + 1];
      // an approximate ideal restriction is not the transpose of P: its natural-order copy is renumbered -- rows by the
      // coarse level's order, columns by this level's positions
      const bool own_R = Lv.restriction_kind != 0;
      if (Lv.sP.nnz > 0 && Lv.sP.nrows == Lv.P.nrows) {
        hipStream_t s = ctx().stream;
        sk::permute(Lv.sP, Lv.perm.empty() ? nullptr : Lv.perm.dev(), map_cols ? dpos(l + 1) : nullptr, Lv.oP, s);
        Lv.sP.release();
        if (own_R) {
          sk::permute(Lv.sR, map_cols ? L[l + 1].perm.dev() : nullptr, has_pos[l] ? dpos(l) : nullptr, Lv.oR, s);
          Lv.sR.release();
        } else {
          sk::transpose(Lv.oP, Lv.oR, s);
        }
        const int pr = Lv.P.nrows, pc = Lv.P.ncols;
        Lv.P = HostCSR();
        Lv.R = HostCSR();
        Lv.P.nrows = Lv.R.ncols = pr;
        Lv.P.ncols = Lv.R.nrows = pc;
      } else {
        HostCSR P2;
        permute(Lv.P, Lv.perm.host(), map_cols ? hpos(l + 1).data() : nullptr, P2);
        Lv.P = std::move(P2);
        if (own_R) {
          static const std::vector<int> identity;
          HostCSR R2;
          permute(Lv.R, map_cols ? L[l + 1].perm.host() : identity, has_pos[l] ? hpos(l).data() : nullptr, R2);
          Lv.R = std::move(R2);
        } else {
          host_transpose(Lv.P, Lv.R);
        }
      }
    } else if (Lv.P.nrows > 0 && !Lv.P.ia.empty() && Lv.R.nrows == 0) {
      host_transpose(Lv.P, Lv.R);  // no renumbering on either side: R was not built yet on the device path
    }
    Lv.sA.release();
    Lv.sP.release();
  }
}

// Non-Galerkin coarse operator (HYPRE_BoomerAMGSetNonGalerkinTol, src/HypreSystem.cpp:161-176): the simplified,
// documented form shared with the oracle (oracle.c sparsify_non_galerkin; HYPRE's par_nongalerkn.c is not restated):
// with m_i = max_{j != i} |a_ij|, an off-diagonal entry is dropped iff |a_ij| < tol * min(m_i, m_j) -- small against
// both rows, so a symmetric operator stays symmetric -- and added to its row's diagonal in stored order (row sums
// are kept).  Kept entries stay in stored order.
namespace hs {
void sparsify_non_galerkin(HostCSR &A, double tol) {
  const int n = A.nrows;
  if (n == 0 || !(tol > 0.0)) return;
  const std::vector<double> m = offdiag_row_maxima(n, A.ia, A.ja, A.a, 0);
  drop_and_lump(n, A.ia, A.ja, A.a, 0, m, [&](int j) { return m[(size_t)j]; }, tol);
}
}  // namespace hs

// ---- internal locality numbering ------------------------------------------------------------------------------
// The x-cache kernels gather, per tile of <= 256 consecutive rows, the tile's unique columns; with a lexicographic
// numbering of a 3-D problem a tile is a piece of ONE grid line and gathers ~5 distinct columns per row, a
// brick-shaped tile ~2.3 (profiles/run_numbering_experiment.py: numbering the same Laplacian by 8x8x8 bricks makes
// the solve 10 % faster per iteration at 256^3).  The geometry is not known here, so compact clusters are grown on
// the matrix graph.  Round 3: graph Voronoi cells instead of sequential breadth-first balls -- rows are cut into
// segments of 2^k consecutive rows (k from the matrix: about four times the typical largest column offset, i.e. four
// z-planes of a lexicographic grid; locality_segment_shift); every row whose hashed index is 0 modulo the cluster size
// (512) is a seed; in rounds, every still unlabelled row takes the smallest label among its neighbours OF ITS SEGMENT
// labelled in the PREVIOUS round (so the result depends neither on threads nor on scheduling), until nothing changes
// (at most 64 rounds; what is farther than that from every seed forms one last cluster in natural order).  The cells
// are then ranked by their smallest row -- a sweep through each segment, so that cells sharing columns stay a few
// cells apart (L2 reuse between neighbouring tiles: a first version ranked the cells by their seeds' indices, which
// scatters neighbouring cells over the whole slab and cost 3.5 GB more HBM traffic per level-0 SpMV at 512^3) -- and
// the rows sorted by cell rank, natural order inside a cell; the coarse levels inherit the order, C points keeping
// their relative order.  Tile statistics equal those of the round-2 balls; the rounds are plain data-parallel
// passes: 512^3 takes tens of milliseconds on the device (sk::locality_labels) where the sequential balls took ~2 s
// of host threads, and the permuted operator is built on the device from the copy HYPRE_IJMatrixAssemble left there.
namespace hs {
const int LOCALITY_CLUSTER = getenv("MI_HYPRE_LOCALITY_CLUSTER") ? std::max(8, atoi(getenv("MI_HYPRE_LOCALITY_CLUSTER"))) : 512;

// Segment length (a power of two, as a shift): about four times the typical largest column offset of a row -- for a
// lexicographic n^3 grid four z-planes.  Cells are confined to segments and ranked in sweep order inside them (below).
int locality_segment_shift(const HostCSR &D) {
  const int n = D.nrows;
  if (getenv("MI_HYPRE_LOCALITY_SEGMENT")) return std::max(8, std::min(30, atoi(getenv("MI_HYPRE_LOCALITY_SEGMENT"))));
  std::vector<int64_t> off;
  const int samples = std::min(n, 4096);
  for (int q = 0; q < samples; q++) {
    const int i = (int)((int64_t)q * n / samples);
    int64_t mx = 0;
    for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++)
      mx = std::max<int64_t>(mx, std::llabs((int64_t)D.ja[(size_t)k] - i));
    off.push_back(mx);
  }
  if (off.empty()) return 20;
  std::nth_element(off.begin(), off.begin() + (long)off.size() / 2, off.end());
  const int64_t want = 4 * std::max<int64_t>(1, off[off.size() / 2]);
  int sh = 14;
  while (sh < 22 && ((int64_t)1 << sh) < want) sh++;
  return sh;
}

// seeds of the clustering in ascending order (exclude: rows that stay out): rows whose hashed index is 0 modulo the
// cluster size; a segment without any gets its first row that takes part
std::vector<int> locality_seeds(int n, int segshift, const std::vector<char> *exclude) {
  const unsigned long long cl = (unsigned long long)LOCALITY_CLUSTER;
  const int nseg = (int)((((int64_t)n - 1) >> segshift) + 1);
  std::vector<std::vector<int>> per_seg((size_t)std::max(nseg, 0));
  parallel_for(nseg, [&](int64_t b, int64_t e, int) {
    for (int64_t sg = b; sg < e; sg++) {
      std::vector<int> &mine = per_seg[(size_t)sg];
      const int64_t r0 = sg << segshift, r1 = std::min<int64_t>(n, (sg + 1) << segshift);
      int first = -1;
      for (int64_t i = r0; i < r1; i++) {
        if (exclude && (*exclude)[(size_t)i]) continue;
        if (first < 0) first = (int)i;
        unsigned long long z = (unsigned long long)i + 0x9E3779B97F4A7C15ULL;  // splitmix64
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        if (z % cl == 0) mine.push_back((int)i);
      }
      if (mine.empty() && first >= 0) mine.push_back(first);
    }
  });
  std::vector<int> seeds;
  for (auto &v : per_seg) seeds.insert(seeds.end(), v.begin(), v.end());
  return seeds;
}

// final labels (cell = seed rank, -1 = never reached, LOCALITY_EXCLUDED) -> order[new] = old.  Cells are ranked by their
// SMALLEST ROW: scanning the rows in the caller's order, a cell takes the next rank when its first row appears.  With
// cells confined to a segment that is a sweep through the segment -- on a lexicographic grid along x, then y, through
// a slab of four planes -- so that cells which share columns are a few cells apart in the new order (what one L2 still
// holds), as the round-2 breadth-first balls were.  Then a stable counting sort of the rows by cell rank; unreached
// rows form one last cluster, excluded rows come last, both in natural order.
void locality_sort(std::vector<int> &label, int nseeds, std::vector<int> &order) {
  const int n = (int)label.size();
  std::vector<int> minrow((size_t)nseeds, n);
  for (int i = n - 1; i >= 0; i--)
    if (label[(size_t)i] >= 0) minrow[(size_t)label[(size_t)i]] = i;
  std::vector<int> cells((size_t)nseeds);
  for (int c = 0; c < nseeds; c++) cells[(size_t)c] = c;
  std::sort(cells.begin(), cells.end(), [&](int a, int b) {
    return minrow[(size_t)a] != minrow[(size_t)b] ? minrow[(size_t)a] < minrow[(size_t)b] : a < b;
  });
  std::vector<int> rank((size_t)nseeds);
  for (int q = 0; q < nseeds; q++) rank[(size_t)cells[(size_t)q]] = q;
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int &l = label[(size_t)i];
      if (l >= 0)
        l = rank[(size_t)l];
      else if (l == -1)
        l = nseeds;
    }
  });
  const int nlab = nseeds + 2;  // cells, the unreached rest, the excluded rows
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (int64_t)n / 65536 + 1));
  std::vector<std::vector<int64_t>> hist((size_t)nt, std::vector<int64_t>((size_t)nlab, 0));
  const int64_t per = ((int64_t)n + nt - 1) / nt;
  auto lab = [&](int i) { return label[(size_t)i] == LOCALITY_EXCLUDED ? nseeds + 1 : label[(size_t)i]; };
  {
    std::vector<std::thread> th;
    auto count = [&](int t) {
      std::vector<int64_t> &h = hist[(size_t)t];
      for (int64_t i = t * per; i < std::min<int64_t>(n, (t + 1) * per); i++) h[(size_t)lab((int)i)]++;
    };
    for (int t = 1; t < nt; t++) th.emplace_back(count, t);
    count(0);
    for (auto &x : th) x.join();
  }
  int64_t run = 0;
  for (int c = 0; c < nlab; c++)
    for (int t = 0; t < nt; t++) {
      const int64_t h = hist[(size_t)t][(size_t)c];
      hist[(size_t)t][(size_t)c] = run;
      run += h;
    }
  order.resize((size_t)n);
  {
    std::vector<std::thread> th;
    auto place = [&](int t) {
      std::vector<int64_t> &h = hist[(size_t)t];
      for (int64_t i = t * per; i < std::min<int64_t>(n, (t + 1) * per); i++) order[(size_t)h[(size_t)lab((int)i)]++] = (int)i;
    };
    for (int t = 1; t < nt; t++) th.emplace_back(place, t);
    place(0);
    for (auto &x : th) x.join();
  }
}

// exclude (optional): rows that stay out of the clustering and come LAST, in natural order (rows with halo
// entries on N > 1 ranks: the halo-free rows then form one stretch that is swept while the halo travels)
void locality_order(const HostCSR &D, std::vector<int> &order, const std::vector<char> *exclude) {
  const int n = D.nrows;
  const int segshift = locality_segment_shift(D);
  const std::vector<int> seeds = locality_seeds(n, segshift, exclude);
  const int nseeds = (int)seeds.size();
  std::vector<int> label((size_t)n, -1);
  if (exclude)
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      for (int64_t i = b; i < e; i++)
        if ((*exclude)[(size_t)i]) label[(size_t)i] = LOCALITY_EXCLUDED;
    });
  for (int k = 0; k < nseeds; k++) label[(size_t)seeds[(size_t)k]] = k;
  std::vector<int> active;
  active.reserve((size_t)n);
  for (int i = 0; i < n; i++)
    if (label[(size_t)i] == -1) active.push_back(i);
  std::vector<int> next;
  for (int round = 0; round < LOCALITY_MAX_ROUNDS && !active.empty(); round++) {
    next.assign(active.size(), -1);
    parallel_for((int64_t)active.size(), [&](int64_t b, int64_t e, int) {
      for (int64_t q = b; q < e; q++) {
        const int i = active[(size_t)q];
        const int sg = i >> segshift;
        int m = -1;
        for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++) {
          const int j = D.ja[(size_t)k];
          if ((j >> segshift) != sg) continue;  // cells do not cross segments
          const int lj = label[(size_t)j];
          if (lj >= 0 && (m < 0 || lj < m)) m = lj;
        }
        next[(size_t)q] = m;
      }
    });
    size_t w = 0;
    for (size_t q = 0; q < active.size(); q++) {
      if (next[q] >= 0)
        label[(size_t)active[q]] = next[q];
      else
        active[w++] = active[q];
    }
    if (w == active.size()) break;  // nothing changed
    active.resize(w);
  }
  locality_sort(label, nseeds, order);
}

// B = Q A Q^T: rows of A in `order` (new -> old), columns renumbered, rows re-sorted
void permute_symmetric(const HostCSR &A, const std::vector<int> &order, HostCSR &B) {
  const int n = A.nrows;
  std::vector<int> newid((size_t)n);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t q = b; q < e; q++) newid[(size_t)order[(size_t)q]] = (int)q;
  });
  B.nrows = n;
  B.ncols = A.ncols;
  B.ia.assign((size_t)n + 1, 0);
  for (int q = 0; q < n; q++) {
    const int i = order[(size_t)q];
    B.ia[(size_t)q + 1] = B.ia[(size_t)q] + (A.ia[(size_t)i + 1] - A.ia[(size_t)i]);
  }
  B.ja.resize((size_t)B.nnz());
  B.a.resize((size_t)B.nnz());
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    std::vector<std::pair<int, double>> row;
    for (int64_t q = b; q < e; q++) {
      const int i = order[(size_t)q];
      row.clear();
      for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) row.push_back({newid[(size_t)A.ja[(size_t)k]], A.a[(size_t)k]});
      std::sort(row.begin(), row.end(), [](const std::pair<int, double> &x, const std::pair<int, double> &y) { return x.first < y.first; });
      int64_t w = B.ia[(size_t)q];
      for (auto &en : row) {
        B.ja[(size_t)w] = en.first;
        B.a[(size_t)w++] = en.second;
      }
    }
  });
}
}  // namespace hs

// one rank: large systems (or MI_HYPRE_LOCALITY_ORDER=1); N > 1 ranks (distributed setup): the same rule on the mean
// rows per rank, so that every rank decides alike
bool BoomerAMG::use_locality_order(const ParCSR &A) const {
  if (forced_comm || A.host_diag_stale) return false;
  const int size = my_comm().size;
  if (size == 1 && !A.col_map_offd.empty()) return false;
  const char *e = getenv("MI_HYPRE_LOCALITY_ORDER");
  if (e && atoi(e) == 0) return false;
  const long long rows = (long long)(A.global_rows() / std::max(1, size));
  if (e && atoi(e) > 0) return rows > 1;
  static const long long min_rows = getenv("MI_HYPRE_LOCALITY_MIN_ROWS") ? atoll(getenv("MI_HYPRE_LOCALITY_MIN_ROWS")) : 1000000;
  return rows >= min_rows;
}

// What a Setup refuses before it builds or refreshes anything: settings that are not implemented (never a substitute)
void BoomerAMG::validate_settings() const {
  if (!coarsen_type_restated(p.coarsen_type))
    fail(4, "BoomerAMGSetup: coarsen_type " + std::to_string(p.coarsen_type) +
                " is not implemented (8 PMIS, 10 HMIS, 11, 6 Falgout, 1, 3, 0 CLJP, 7 are); refusing to substitute another one");
  if (p.agg_num_levels > 0 && p.agg_interp_type != 4 && p.agg_interp_type != 5)
    fail(4, "BoomerAMGSetup: agg_interp_type " + std::to_string(p.agg_interp_type) +
                " is not implemented (4 = multipass and 5 = two-stage extended are); refusing to substitute another one");
  for (int k = 0; k < 3; k++) {
    const int t = p.relax_type[k];
    const bool known = t == 0 || t == 7 || t == 18 || t == 3 || t == 4 || t == 6 || t == 8 || t == 13 || t == 14 ||
                       t == 11 || t == 12 || t == 9 || t == 16 || is_mcgs(t);
    if (!known)
      fail(4, "BoomerAMGSetup: relax_type " + std::to_string(t) +
                  " is not implemented (0, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14, 16, 18, 40, 41, 42 are); refusing to smooth with "
                  "something else");
    if (is_mcgs(t) && my_comm().size > 1)
      fail(4, "BoomerAMGSetup: relax_type " + std::to_string(t) + " (multicolour Gauss-Seidel) is not implemented on more than "
                  "one rank (" + std::to_string(my_comm().size) + " ranks); refusing to smooth with something else");
    if (is_mcgs(t) && host_only)
      fail(4, "BoomerAMGSetup: relax_type " + std::to_string(t) + " (multicolour Gauss-Seidel) is not implemented by the "
                  "host-only setup (the colouring is device code); refusing to smooth with something else");
    if (t == 16 && host_only)
      fail(4, "BoomerAMGSetup: relax_type 16 (Chebyshev) is not implemented by the host-only setup, which has no eigenvalue "
              "estimate (that is device code); refusing to smooth with something else");
    // 9 = direct solve: the coarsest level only (BoomerAMG::relax would otherwise have to smooth the other
    // levels with something else, or fail inside the Krylov loop)
    if (t == 9 && k < 2)
      fail(4, std::string("BoomerAMGSetup: relax_type 9 (Gaussian elimination) is implemented for the coarsest level only, not as the ") +
                  (k == 0 ? "down" : "up") + " smoother; refusing to smooth with something else");
  }
  if (wants_cheby()) {
    if (p.cheby_order < 1 || p.cheby_order > 4)
      fail(4, "BoomerAMGSetup: Chebyshev order " + std::to_string(p.cheby_order) +
                  " is not implemented (1, 2, 3 and 4 are); refusing to smooth with another polynomial");
    if (!(p.cheby_fraction > 0.0 && p.cheby_fraction < 1.0))
      fail(4, "BoomerAMGSetup: Chebyshev eigenvalue fraction " + std::to_string(p.cheby_fraction) +
                  " is not implemented (a value strictly between 0 and 1 is); refusing to smooth on another interval");
    if (p.cheby_eig_est < 0)
      fail(4, "BoomerAMGSetup: Chebyshev eig_est " + std::to_string(p.cheby_eig_est) +
                  " is not implemented (0 = Gershgorin and k > 0 CG steps are); refusing to estimate another way");
    if (p.cheby_variant != 0)
      fail(4, "BoomerAMGSetup: Chebyshev variant " + std::to_string(p.cheby_variant) +
                  " is not implemented (0 is); refusing to smooth with another variant");
    if (p.cheby_scale != 1)
      fail(4, "BoomerAMGSetup: Chebyshev scale " + std::to_string(p.cheby_scale) +
                  " is not implemented (1 = the diagonally scaled operator is); refusing to smooth the unscaled one");
  }
  if (p.interp_type != 0 && p.interp_type != 3 && p.interp_type != 4 && p.interp_type != 6 && p.interp_type != 16 &&
      p.interp_type != 17 && p.interp_type != 100)
    fail(4, "BoomerAMGSetup: interp_type " + std::to_string(p.interp_type) +
                " is not implemented (0 classical modified, 3 direct, 4 multipass, 6 extended+i, 16 extended and 17 extended+i in "
                "matrix-matrix form, 100 one-point are); refusing to substitute another one");
  if (p.restriction != 0 && p.restriction != 1)
    fail(4, "BoomerAMGSetup: restriction " + std::to_string(p.restriction) +
                " is not implemented (0 = the transpose of P and 1 = distance-1 approximate ideal restriction are); refusing "
                "to substitute another one");
  // (the two thresholds are refused whatever the restriction: a handle that holds one would build another R once
  // restriction 1 is set)
  if (!(p.strong_threshold_r >= 0.0))
    fail(4, "BoomerAMGSetup: strong_threshold_r " + std::to_string(p.strong_threshold_r) +
                " is not implemented (a value >= 0 is); refusing to build the restriction on another graph");
  if (!(p.filter_threshold_r >= 0.0))
    fail(4, "BoomerAMGSetup: filter_threshold_r " + std::to_string(p.filter_threshold_r) +
                " is not implemented (a value >= 0 is); refusing to filter the restriction another way");
  if (p.restriction == 1) {
    if (p.agg_num_levels > 0)
      fail(4, "BoomerAMGSetup: restriction 1 (approximate ideal restriction) with agg_num_levels " +
                  std::to_string(p.agg_num_levels) + " is not implemented (it is on levels that are not aggressive); refusing "
                  "to restrict an aggressive level with the transpose of P");
    if (my_comm().size > 1)
      fail(4, "BoomerAMGSetup: restriction 1 (approximate ideal restriction) is not implemented on more than one rank (" +
                  std::to_string(my_comm().size) + " ranks); refusing to restrict with the transpose of P");
  }
  if (p.num_functions < 1)
    fail(4, "BoomerAMGSetup: num_functions " + std::to_string(p.num_functions) +
                " is not implemented (a value >= 1 is); refusing to treat the system as a scalar problem");
  if (p.num_functions > 1) {
    if (p.restriction == 1)
      fail(4, "BoomerAMGSetup: restriction 1 (approximate ideal restriction) with num_functions " +
                  std::to_string(p.num_functions) + " is not implemented (it is with num_functions 1); refusing to restrict "
                  "with the transpose of P");
    if (my_comm().size > 1)
      fail(4, "BoomerAMGSetup: num_functions " + std::to_string(p.num_functions) + " is not implemented on more than one rank (" +
                  std::to_string(my_comm().size) + " ranks); refusing to treat the system as a scalar problem");
  }
  if (p.smooth_num_levels > 0 && p.smooth_type != 5 && p.smooth_type != 4)
    fail(4, "BoomerAMGSetup: smooth_type " + std::to_string(p.smooth_type) + " on " + std::to_string(p.smooth_num_levels) +
                " level(s) is not implemented (4 = FSAI and 5 = ILU are); refusing to smooth with something else");
  if (p.smooth_num_levels > 0 && p.smooth_type == 4 && p.fsai_algo_type != 3 && p.fsai_algo_type != 4)
    fail(4, "BoomerAMGSetup: FSAI algo_type " + std::to_string(p.fsai_algo_type) +
                " is not implemented (3 = static pattern and 4 = adaptive pattern are); refusing to substitute another one");
  if (p.smooth_num_levels > 0 && p.smooth_type == 4 && p.fsai_algo_type == 4)
    FsaiSolver::check_adaptive("BoomerAMGSetup", p.fsai_max_steps, p.fsai_max_step_size, p.fsai_kap_tolerance);
  if (p.smooth_num_levels > 0 && p.smooth_type == 4 && p.fsai_algo_type == 3 && (p.fsai_num_levels < 1 || p.fsai_num_levels > 3))
    fail(4, "BoomerAMGSetup: FSAI num_levels " + std::to_string(p.fsai_num_levels) + " is not implemented (1, 2 and 3 are)");
  if (p.smooth_num_levels > 0 && p.smooth_type == 5 && (p.ilu_type != 0 || p.ilu_level < 0))
    fail(4, "BoomerAMGSetup: ILU smoother type " + std::to_string(p.ilu_type) + " / level of fill " +
                std::to_string(p.ilu_level) + " is not implemented (block-Jacobi ILU(k) = type 0, level k >= 0 is)");
  if (p.smooth_num_levels > 0 && p.smooth_type == 5 && p.ilu_iter_type != 0 &&
      (p.ilu_iter_type < 0 || p.ilu_iter_type > 4 || p.ilu_level != 0 || (p.ilu_iter_option & ~63) || p.ilu_iter_max_iter < 1))
    fail(4, "BoomerAMGSetup: iterative ILU setup type " + std::to_string(p.ilu_iter_type) + " with level of fill " +
                std::to_string(p.ilu_level) + ", option " + std::to_string(p.ilu_iter_option) + ", max iterations " +
                std::to_string(p.ilu_iter_max_iter) +
                " is not implemented (types 0 ... 4 with ILU(0), option bits 1 ... 32, max iterations >= 1 are)");
}

// num_functions > 1: the caller's dof_func (or the interleaved default) of this rank's rows, copied and checked
void BoomerAMG::read_dof_func(const ParCSR &A0) {
  const size_t n = (size_t)A0.nrows;
  const int k = p.num_functions;
  pending_dof.resize(n);
  if (!dof_func_user) {
    for (size_t i = 0; i < n; i++) pending_dof[i] = (int)((A0.row_start + (gidx)i) % (gidx)k);
    return;
  }
  if (n && is_device_pointer(dof_func_user))
    d2h(pending_dof.data(), dof_func_user, n * sizeof(int), nullptr);
  else if (n)
    memcpy(pending_dof.data(), dof_func_user, n * sizeof(int));
  for (size_t i = 0; i < n; i++)
    if (pending_dof[i] < 0 || pending_dof[i] >= k)
      fail(4, "BoomerAMGSetup: dof_func[" + std::to_string(i) + "] = " + std::to_string(pending_dof[i]) +
                  " (local row " + std::to_string(i) + ") is outside [0, num_functions = " + std::to_string(k) +
                  "); refusing to guess the row's unknown");
}

void BoomerAMG::setup_host(ParCSR &A0) {
  TraceRange trace_setup("mi_hypre BoomerAMGSetup (hierarchy)");
  Comm &comm = my_comm();
  t_setup_start = wall_time();
  for (double &t : t_phase) t = 0.0;
  is_setup = false;
  host_ready = false;
  MI_REQUIRE(!A0.row_starts.empty(), "BoomerAMGSetup: matrix is not assembled");
  validate_settings();
  if (device_min_rows >= 0) dev_arena_hint((size_t)13 * 12 * (size_t)(A0.diag_nnz() + A0.offd.nnz()));
  if (comm.size > 1) input_order.clear();
  if (comm.size > 1 && can_build_distributed()) {
    build_distributed(A0);
  } else if (comm.size > 1) {
    build_replicated(A0);
  } else {
    tail.reset();
    tail_A.reset();
    input_order.clear();
    Aq_own.reset();
    ParCSR *Ain = &A0;
    pending_sA0.release();
    if (use_locality_order(A0)) {
      TraceRange trace_q("setup: internal numbering");
      const double tq0 = wall_time();
      Aq_own.reset(new ParCSR());
      ParCSR &Q = *Aq_own;
      const int n0 = A0.nrows;
      // on the device when the level will be built there anyway: the clustering rounds are data-parallel passes,
      // and Q A Q^T is permuted from the copy HYPRE_IJMatrixAssemble left in HBM -- neither the host's copy of the
      // permuted operator (0.94 G entries at 512^3) nor its upload exist any more
      const bool on_dev = device_min_rows >= 0 && n0 >= device_min_rows && A0.on_device && A0.d_diag.nrows == n0 &&
                          A0.d_diag.nnz == A0.diag.nnz() && !A0.d_diag.rowmap.p;
      if (on_dev) {
        hipStream_t s = ctx().stream;
        sk::DCsr raw;
        std::unique_ptr<TraceRange> tr(new TraceRange("numbering: plain CSR copy + segment length"));
        sk::from_solve_format(A0.d_diag, raw, s);
        const int segshift = locality_segment_shift(A0.diag);
        tr.reset(), tr.reset(new TraceRange("numbering: seeds, label rounds, order (device)"));
        // seeds, rounds, cell ranks and the rows' order all on the device (round 4; the labels used to travel to the host
        // for a counting sort there, the order back: ~0.6 s of host time at 512^3)
        DVec<int> dorder;
        int nseeds = 0, rounds = 0;
        if (!sk::locality_order_device(raw, segshift, LOCALITY_CLUSTER, LOCALITY_MAX_ROUNDS, dorder, nseeds, rounds, s)) {
          const std::vector<int> seeds = locality_seeds(n0, segshift, nullptr);
          std::vector<int> label, order_h;
          rounds = sk::locality_labels(raw, seeds.data(), (int)seeds.size(), nullptr, segshift, LOCALITY_MAX_ROUNDS, label, s);
          nseeds = (int)seeds.size();
          locality_sort(label, nseeds, order_h);
          dorder.upload(order_h);
        }
        tr.reset(), tr.reset(new TraceRange("numbering: Q A Q^T"));
        DVec<int> dpos((size_t)n0);
        sk::invert_permutation(dorder.p, n0, dpos.p, s);
        sk::permute(raw, dorder.p, dpos.p, pending_sA0, s);
        MI_HIP(hipStreamSynchronize(s));
        input_order.adopt_device(std::move(dorder), (size_t)n0);
        tr.reset();
        Q.diag.nrows = Q.diag.ncols = n0;
        Q.host_diag_stale = true;
        Q.dev_diag_nnz = pending_sA0.nnz;
        if (getenv("MI_HYPRE_SETUP_TIMING"))
          printf("   locality numbering on the device: segments of 2^%d rows, %d seeds, %d rounds\n", segshift, nseeds, rounds);
      } else {
        std::vector<int> order_h;
        locality_order(A0.diag, order_h, nullptr);
        permute_symmetric(A0.diag, order_h, Q.diag);
        input_order = std::move(order_h);
      }
      Q.nrows = A0.nrows;
      Q.row_start = A0.row_start;
      Q.row_end = A0.row_end;
      Q.row_starts = A0.row_starts;
      Q.offd.nrows = A0.nrows;
      Q.offd.ncols = 0;
      if (!Q.host_diag_stale) Q.offd.ia.assign((size_t)A0.nrows + 1, 0);  // (device-resident: ParCSR::ensure_offd_rows)
      Q.build_halo_plan(comm);
      Ain = Aq_own.get();
      if (getenv("MI_HYPRE_SETUP_TIMING")) printf("   locality numbering of the input: %.2f s\n", wall_time() - tq0);
    }
    pending_dof.clear();
    if (p.num_functions > 1) {
      read_dof_func(A0);
      if (!input_order.empty()) {  // the hierarchy is built on Q A Q^T: row q of it is the caller's row input_order[q]
        const std::vector<int> &oh = input_order.host();
        std::vector<int> q(pending_dof.size());
        for (size_t i = 0; i < q.size(); i++) q[i] = pending_dof[(size_t)oh[i]];
        pending_dof.swap(q);
      }
    }
    build_natural(*Ain);
    const double tp0 = wall_time();
    {
      TraceRange tr("setup: C-first ordering");
      apply_cf_ordering();
    }
    TraceRange trace_w("setup: transfer operator wrappers + level-0 permutation");
    make_local_transfer_operators();
    if (!input_order.empty()) {
      // level 0 rows -> caller rows
      AmgLevel &L0 = L[0];
      if (L0.perm.empty()) {
        L0.perm = input_order.host();
      } else if (L0.perm.on_device() && input_order.on_device()) {
        const size_t n = L0.perm.size();
        DVec<int> composed(n);
        sk::gather_elems(input_order.dev(), L0.perm.dev(), 0, (int)n, 4, composed.p, ctx().stream);
        MI_HIP(hipStreamSynchronize(ctx().stream));
        L0.perm.adopt_device(std::move(composed), n);
      } else {
        const std::vector<int> &oh = input_order.host();
        std::vector<int> &ph = L0.perm.hostw();
        parallel_for((int64_t)ph.size(), [&](int64_t b, int64_t e, int) {
          for (int64_t q = b; q < e; q++) ph[(size_t)q] = oh[(size_t)ph[(size_t)q]];
        });
      }
      if (L0.A != Aq_own.get()) Aq_own.reset();  // level 0 is its C-first copy: the intermediate matrix can go
    }
    t_phase[4] += wall_time() - tp0;
  }
  {
    TraceRange tr("setup: norms + coarsest inverse");
    finish_host();
  }
  global_opcx = -1.0;
  if (comm.size > 1 && !L.empty()) {  // the operator complexity HYPRE would print: summed over the ranks, here where all are present
    double v[2] = {0.0, 0.0};
    local_entry_counts(v[0], v[1]);
    comm.allreduce_host(v, 2, CommDType::F64, CommOp::SUM);
    global_opcx = v[1] > 0 ? v[0] / v[1] : 0.0;
  }
  t_phase[5] = wall_time() - t_setup_start;
  host_ready = true;
  if (getenv("MI_HYPRE_SETUP_TIMING") && comm.rank == 0)
    // (wall time per phase of the hierarchy build; on levels the device builds this is kernel time -- the split into
    // device-busy and device-idle time comes from a trace: profiles/setup_split.py)
    printf("mi_hypre hierarchy build (wall per phase): strength %.2f  pmis %.2f  interp %.2f  galerkin %.2f  ordering/slicing %.2f  total %.2f s\n",
           t_phase[0], t_phase[1], t_phase[2], t_phase[3], t_phase[4], t_phase[5]);
}

// ---- the single-rank level build ("The level build") --------------------------------------------
// which routine makes a level's P: resolved once per level, switched on by the device and by the host dispatch
enum class InterpKind { classical, multipass, two_stage, mm_ext, one_point };
static InterpKind interp_kind(bool aggressive, const AmgParams &p) {
  // aggressive levels: multipass (agg_interp_type 4) or the two-stage extended interpolation (5; validate_settings)
  if (aggressive) return p.agg_interp_type == 5 ? InterpKind::two_stage : InterpKind::multipass;
  switch (p.interp_type) {
    case 4: return InterpKind::multipass;  // on an ordinary splitting its first pass is all there is, unless F points
                                           // lack a strong C point
    case 16:
    case 17: return InterpKind::mm_ext;  // the matrix-matrix extended interpolations
    case 100: return InterpKind::one_point;
    default: return InterpKind::classical;  // 0, 6 (sk::interp on a device level) and 3: build_interp
  }
}

// A C/F marker of the level being built: on the host, on the device, or -- the same contents -- on both.  host() / dev()
// copy across when only the other side holds it; a routine that rewrites the marker asks for its side alone.
struct LevelMarker {
  std::vector<int> h;
  DVec<int> d;
  bool host_ok = false, dev_ok = false;
  std::vector<int> &fill_host() { return host_ok = true, dev_ok = false, h; }
  DVec<int> &fill_dev() { return dev_ok = true, host_ok = false, d; }
  std::vector<int> &host() {
    if (!host_ok) h = d.to_host();
    return host_ok = true, h;
  }
  DVec<int> &dev() {
    if (!dev_ok) d.upload(h);
    return dev_ok = true, d;
  }
  std::vector<int> &host_only() {
    host();
    d.release();
    return dev_ok = false, h;
  }
  DVec<int> &dev_only() {
    dev();
    return host_ok = false, d;
  }
};

// What build_natural knows about the level it is building: the strength graph and the marker(s) with the side that
// holds them, where P and R ended up, and the clock of the phase accounting.
struct LevelBuild {
  const int l, n;
  ParCSR &A;
  AmgLevel &Lv;
  const bool on_device, aggressive;
  const InterpKind kind;
  // aggressive coarsening and the Ruge-Stueben family are host algorithms: on a level the device builds, the strength
  // graph still comes from the device and the Galerkin product stays there.  (With the two-stage interpolation and PMIS
  // the aggressive level stays on the device: second graph, second PMIS, marker correction, the sparse products.)
  const bool host_coarsen;
  Strength S;  // the strength graph: the device builds dS and S is its copy, the host builds S alone
  sk::DCsr dS;
  bool S_on_host = false;
  LevelMarker cf, cf1;  // cf1: the marker after the first coarsening of an aggressive level (two-stage interpolation)
  // num_functions > 1: the same-function operator F(A) that steps 1 and 2 read in A's place -- dF on a device level, F
  // for the host routines (made from dF when a device level hands its interpolation to one); gone after step 2
  const bool systems;
  sk::DCsr dF;
  std::unique_ptr<ParCSR> F;
  LazyInts dof_coarse;  // the coarse level's dof_func (end of step 2), handed to the new level by build_natural
  bool p_on_device = false;
  int nc = 0;
  sk::DCsr dR_local, *dR = nullptr;  // the device's R for the Galerkin product (Lv.sR where it is kept)
  double tp0 = 0.0, t_filter = 0.0;
  std::unique_ptr<TraceRange> trace;

  LevelBuild(int level, AmgLevel &lv, const AmgParams &p, long long device_min_rows)
      : l(level), n(lv.A->nrows), A(*lv.A), Lv(lv), on_device(device_min_rows >= 0 && n >= device_min_rows),
        aggressive(level < p.agg_num_levels), kind(interp_kind(aggressive, p)),
        host_coarsen(!on_device || !(p.coarsen_type == 8 || p.coarsen_type == 9) ||
                     (aggressive && kind != InterpKind::two_stage)),
        systems(p.num_functions > 1) {}
  // the operator whose strength graph, splitting and interpolation the level gets
  const sk::DCsr &graph_operator_dev() const { return systems ? dF : Lv.sA; }
  ParCSR &graph_operator_host() {
    if (!systems) return A;
    if (!F) {
      F.reset(new ParCSR());
      if (on_device)
        dF.download(F->diag, ctx().stream);
      else
        filter_same_function(A.diag, Lv.dof.host(), F->diag);
      F->diag.nrows = F->diag.ncols = n;
      F->nrows = n;
      F->row_start = 0;
      F->row_end = n;
      F->row_starts = {0, (gidx)n};
      F->offd.nrows = n;
      F->offd.ncols = 0;
      F->offd.ia.assign((size_t)n + 1, 0);
    }
    return *F;
  }
  void begin(const char *what) {
    trace.reset(), trace.reset(new TraceRange(("level " + std::to_string(l) + ": " + what).c_str()));
  }
  double lap() {  // seconds since the last lap
    const double t = wall_time(), dt = t - tp0;
    return tp0 = t, dt;
  }
  const Strength &strength_to_host() {
    if (!S_on_host) {
      hipStream_t s = ctx().stream;
      S.ia.resize((size_t)n + 1);
      S.ja.resize((size_t)dS.nnz);
      d2h(S.ia.data(), dS.ia.p, ((size_t)n + 1) * sizeof(int64_t), s);
      if (dS.nnz) d2h(S.ja.data(), dS.ja.p, (size_t)dS.nnz * sizeof(int), s);
      MI_HIP(hipStreamSynchronize(s));
      S_on_host = true;
    }
    return S;
  }
  long long count_c_points() {
    if (!cf.host_ok) {
      DVec<long long> crank;
      return sk::count_c_points(cf.d.p, n, crank, ctx().stream);
    }
    std::atomic<long long> acc{0};
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      long long c = 0;
      for (int64_t i = b; i < e; i++) c += (cf.h[(size_t)i] == C_PT);
      acc += c;
    });
    return acc.load();
  }
};

// the host arrays of an operator only the device holds (dev: its plain CSR copy, else the solve format is read back)
void BoomerAMG::fetch_operator(ParCSR *M, sk::DCsr &dev) {
  if (!M || !M->host_diag_stale) return;
  hipStream_t s = ctx().stream;
  const int nr = M->diag.nrows, ncl = M->diag.ncols;
  if (dev.nrows == M->nrows && dev.ia.p)
    dev.download(M->diag, s);
  else
    sk::solve_format_to_host(M->d_diag, M->diag, s);
  M->diag.nrows = nr;
  M->diag.ncols = ncl;
  M->host_diag_stale = false;
  M->ensure_offd_rows();
}

// step 0 (num_functions > 1 only): the same-function operator F(A) of the level, from the level's dof_func
void BoomerAMG::level_same_function_operator(LevelBuild &b) {
  if (!b.systems) return;
  MI_REQUIRE(b.Lv.dof.size() == (size_t)b.n, "level build: the level has no dof_func");
  double t0 = wall_time();
  if (b.on_device) {
    hipStream_t s = ctx().stream;
    if (b.Lv.sA.nrows != b.n) b.Lv.sA.upload(b.A.diag, s);  // (what step 1 would upload; not the filter's time)
    const int *dof = b.Lv.dof.dev();
    t0 = wall_time();
    sk::same_function_filter(b.Lv.sA, dof, b.dF, s);
  } else {
    b.graph_operator_host();
  }
  b.t_filter = wall_time() - t0;
}

// step 1: the strength graph and the splitting; leaves the level's marker in b.cf (and b.cf1)
void BoomerAMG::level_strength_and_coarsening(LevelBuild &b) {
  double t_strength = 0.0;
  if (b.on_device) {
    // strength graph and PMIS splitting on the device (integer/compare work, identical results)
    hipStream_t s = ctx().stream;
    if (b.Lv.sA.nrows != b.n) b.Lv.sA.upload(b.A.diag, s);
    const double ts0 = wall_time();
    sk::strength(b.graph_operator_dev(), p.strong_threshold, p.max_row_sum, b.dS, s);
    t_strength = wall_time() - ts0;
  } else {
    const double ts0 = wall_time();
    strength(b.graph_operator_host(), p.strong_threshold, p.max_row_sum, b.S);
    t_strength = wall_time() - ts0;
    b.S_on_host = true;
  }
  t_phase[0] += b.lap();
  if (b.systems && getenv("MI_HYPRE_SETUP_TIMING"))  // (both routines are complete on return: wall time is their time)
    printf("   level %d: n %d  same-function filter %.4f s, strength %.4f s%s\n", b.l, b.n, b.t_filter, t_strength,
           b.on_device ? "" : "  (host routines)");
  const bool two_stage = b.kind == InterpKind::two_stage;
  if (b.host_coarsen) {
    const Strength &S = b.strength_to_host();
    if (b.aggressive)
      coarsen_aggressive(p.coarsen_type, b.n, S, b.cf.fill_host(), two_stage ? &b.cf1.fill_host() : nullptr);
    else
      coarsen_by_type(p.coarsen_type, b.n, S, b.cf.fill_host());
    if (b.on_device) b.cf.dev();
  } else {
    hipStream_t s = ctx().stream;
    sk::pmis(b.dS, 2747, b.cf.fill_dev(), s);  // (the marks stay on the device: LazyInts)
    if (b.aggressive) {
      b.cf1.fill_dev().alloc((size_t)b.n);
      MI_HIP(hipMemcpyAsync(b.cf1.d.p, b.cf.d.p, (size_t)b.n * sizeof(int), hipMemcpyDeviceToDevice, s));
      sk::aggressive_second_stage(b.dS, b.cf.d, 2747, s);
    }
  }
  t_phase[1] += b.lap();
}

// step 2: P of the level by the routine of its kind, on the device where the level lives there; the final marker goes
// to Lv.cf
void BoomerAMG::level_interpolation(LevelBuild &b) {
  AmgLevel &Lv = b.Lv;
  const int n = b.n;
  if (b.kind == InterpKind::two_stage && p.keep_agg_markers) {
    // (inspection, HYPRE_MI_BoomerAMGGetLevelAggMarkers: natural order, before the interpolation rewrites -3)
    const std::vector<int> &h1 = b.cf1.host(), &h2 = b.cf.host();
    Lv.agg_m1.assign(h1.begin(), h1.end());
    Lv.agg_m2.assign(h2.begin(), h2.end());
  }
  int bad = -1;  // a row with a zero denominator (two_stage, mm_ext)
  if (b.on_device) {
    hipStream_t s = ctx().stream;
    const sk::DCsr &dA = b.graph_operator_dev();
    switch (b.kind) {
      case InterpKind::classical:
        if (p.interp_type == 6 || p.interp_type == 0) {  // (declines a row whose interpolatory set outgrows its tables)
          b.p_on_device = sk::interp(dA, b.dS, b.cf.dev(), p.interp_type, p.trunc_factor, p.pmax_elmts, Lv.sP, b.nc, s,
                                     &Lv.interp_census);
          Lv.interp_by_host = false;
        }
        break;
      case InterpKind::multipass: break;  // a host routine
      case InterpKind::two_stage:  // (after a coarsening the host ran, too: the interpolation is the device's all the same)
        bad = sk::two_stage_ext(dA, b.dS, b.cf1.dev(), b.cf.dev(), p.agg_p12_trunc_factor, p.agg_p12_max_elmts,
                                p.agg_trunc_factor, p.agg_pmax_elmts, Lv.sP, b.nc, s);
        b.cf1 = LevelMarker();  // (the first stage's marker has served)
        b.p_on_device = true;
        break;
      case InterpKind::mm_ext:  // two operand builders and sk::spgemm: rows of any length stay on the device
        bad = sk::mm_interp(dA, b.dS, b.cf.dev(), p.interp_type, p.trunc_factor, p.pmax_elmts, Lv.sP, b.nc, s);
        b.p_on_device = true;
        break;
      case InterpKind::one_point:  // one row per lane: rows of any length stay on the device
        sk::one_point_interp(dA, b.dS, b.cf.dev(), Lv.sP, b.nc, s);
        b.p_on_device = true;
        break;
    }
    if (b.p_on_device) {
      // stays on the device; the dimensions are all the host needs
      Lv.P = HostCSR();
      Lv.P.nrows = n;
      Lv.P.ncols = b.nc;
    } else {
      // the host routine runs on the host's copies of the operator, the graph and the marker
      if (!b.systems) fetch_operator(&b.A, Lv.sA);
      b.strength_to_host();
      b.cf.host_only();
    }
    b.dS.release();
  }
  if (!b.p_on_device) {
    std::vector<int> &cf = b.cf.host();
    ParCSR &A = b.graph_operator_host();
    switch (b.kind) {
      case InterpKind::classical: build_interp(A, b.S, cf, p.interp_type, p.trunc_factor, p.pmax_elmts, Lv.P, b.nc); break;
      case InterpKind::multipass:
        build_multipass(A, b.S, cf, b.aggressive ? p.agg_trunc_factor : p.trunc_factor,
                        b.aggressive ? p.agg_pmax_elmts : p.pmax_elmts, Lv.P, b.nc);
        break;
      case InterpKind::two_stage:
        bad = build_two_stage_ext(A, b.S, b.cf1.host(), cf, p.agg_p12_trunc_factor, p.agg_p12_max_elmts, p.agg_trunc_factor,
                                  p.agg_pmax_elmts, Lv.P, b.nc);
        break;
      case InterpKind::mm_ext: bad = build_mm_interp(A, b.S, cf, p.interp_type, p.trunc_factor, p.pmax_elmts, Lv.P, b.nc); break;
      case InterpKind::one_point: build_one_point_interp(A.diag, b.S, cf, Lv.P, b.nc); break;
    }
  }
  if (bad >= 0 && b.kind == InterpKind::two_stage) two_stage_zero_denominator(b.l, bad);
  if (bad >= 0) mm_interp_zero_denominator(p.interp_type, b.l, bad);
  if (b.p_on_device)
    Lv.cf.adopt_device(std::move(b.cf.dev_only()), (size_t)n);  // (interpolation has updated the marks there: -3 -> -1)
  else
    Lv.cf = std::move(b.cf.host_only());
  Lv.has_cf = true;
  if (b.systems) {
    // F(A) has served (the Galerkin product allocates next); the coarse level's dof_func is this one's at the C points
    b.dF.release();
    b.F.reset();
    if (Lv.cf.on_device()) {
      DVec<int> dc;
      sk::gather_at_c_points(Lv.cf.dev(), Lv.dof.dev(), n, dc, ctx().stream);
      b.dof_coarse.adopt_device(std::move(dc), (size_t)b.nc);
    } else {
      const std::vector<int> &cfh = Lv.cf.host(), &dh = Lv.dof.host();
      std::vector<int> dc;
      dc.reserve((size_t)b.nc);
      for (int i = 0; i < n; i++)
        if (cfh[(size_t)i] == C_PT) dc.push_back(dh[(size_t)i]);
      b.dof_coarse = std::move(dc);
    }
  }
}

// step 3: R where the Galerkin product reads it -- Lv.R on a host level, *b.dR on a device level.  The transpose of P,
// or (restriction 1) the approximate ideal restriction, which the device leaves to the host routine when a
// neighbourhood outgrows its 64-lane solve
void BoomerAMG::level_restriction(LevelBuild &b) {
  AmgLevel &Lv = b.Lv;
  const bool air = p.restriction == 1;
  Lv.restriction_kind = 0;
  Lv.air_info = sk::AirInfo();
  if (!b.on_device) {
    if (air) {
      build_air_restriction(b.A.diag, Lv.cf.host(), p.strong_threshold_r, p.filter_threshold_r, Lv.R, Lv.air_info);
      Lv.restriction_kind = 2;
    } else {
      host_transpose(Lv.P, Lv.R);
    }
  } else {
    hipStream_t s = ctx().stream;
    if (!b.p_on_device) Lv.sP.upload(Lv.P, s);  // (a host routine's P: the transpose and the products read the device's copy)
    // the replicated setup slices R on the device later; an approximate ideal restriction is renumbered, not rebuilt
    b.dR = (keep_natural_R || air) ? &Lv.sR : &b.dR_local;
    if (air) {
      const int rc = sk::air_restriction(Lv.sA, Lv.cf.dev(), p.strong_threshold_r, p.filter_threshold_r, *b.dR, Lv.air_info, s);
      Lv.restriction_kind = 1;
      if (rc == 1) {
        fetch_operator(&b.A, Lv.sA);
        HostCSR Rh;
        if (build_air_restriction(b.A.diag, Lv.cf.host(), p.strong_threshold_r, p.filter_threshold_r, Rh, Lv.air_info) < 0)
          b.dR->upload(Rh, s);
        Lv.restriction_kind = 2;
      }
    } else {
      sk::transpose(Lv.sP, *b.dR, s);
    }
  }
  if (Lv.air_info.bad_row >= 0) air_singular_system(b.l, Lv.air_info.bad_row);
}

// step 4: A_c = R (A P), its non-Galerkin sparsification, and the coarse level's entry in L
void BoomerAMG::level_galerkin_and_adopt(LevelBuild &b) {
  AmgLevel &Lv = b.Lv;
  const int l = b.l, nc = b.nc;
  std::unique_ptr<ParCSR> An(new ParCSR());
  if (b.on_device) {
    // same arithmetic, same order (setup_kernels.hip); the natural-order device copies stay for the
    // C-first renumbering
    hipStream_t s = ctx().stream;
    sk::DCsr dAP;
    sk::spgemm(Lv.sA, Lv.sP, dAP, s);
    L.emplace_back();  // the coarse operator is born on the device (L was reserved: references stay valid)
    sk::DCsr &dAc = L[(size_t)l + 1].sA;
    sk::spgemm(*b.dR, dAP, dAc, s);
    if (p.non_galerkin_tol_for(l) > 0.0) sk::sparsify_non_galerkin(dAc, p.non_galerkin_tol_for(l), s);
    if (nc < device_min_rows) {
      dAc.download(An->diag, s);  // the next level is built by the host routines
    } else {
      An->diag.nrows = An->diag.ncols = nc;
      An->host_diag_stale = true;
      An->dev_diag_nnz = dAc.nnz;
    }
    if (getenv("MI_HYPRE_SETUP_TIMING"))
      printf("   level %d: n %d  device Galerkin %.2f s (nnz A %lld, P %lld, AP %lld, A_c %lld)\n", l, b.n, wall_time() - b.tp0,
             (long long)Lv.sA.nnz, (long long)Lv.sP.nnz, (long long)dAP.nnz, (long long)dAc.nnz);
  } else {
    HostCSR AP;
    host_spgemm(b.A.diag, Lv.P, AP);
    host_spgemm(Lv.R, AP, An->diag);
    if (p.non_galerkin_tol_for(l) > 0.0) sparsify_non_galerkin(An->diag, p.non_galerkin_tol_for(l));
    L.emplace_back();
  }
  An->nrows = nc;
  An->row_start = 0;
  An->row_end = nc;
  An->row_starts = {0, (gidx)nc};
  An->offd.nrows = nc;
  An->offd.ncols = 0;
  if (!An->host_diag_stale) An->offd.ia.assign((size_t)nc + 1, 0);  // (device-resident: ParCSR::ensure_offd_rows)
  An->build_halo_plan(my_comm());
  t_phase[3] += b.lap();
  L[(size_t)l + 1].A_own = std::move(An);
  L[(size_t)l + 1].A = L[(size_t)l + 1].A_own.get();
}

// the coarsening loop in natural ordering (single communicator rank, or the
// global operator in the replicated multi-rank setup)
void BoomerAMG::build_natural(ParCSR &A0) {
  Comm &comm = my_comm();
  MI_REQUIRE(comm.size == 1 && A0.col_map_offd.empty(), "build_natural expects a single-rank operator");
  L.clear();
  L.reserve((size_t)std::max(1, p.max_levels));
  L.emplace_back();
  L[0].A = &A0;
  if (pending_sA0.nrows == A0.nrows && pending_sA0.nrows > 0 && A0.host_diag_stale) L[0].sA = std::move(pending_sA0);
  pending_sA0.release();
  if (p.num_functions > 1) L[0].dof = std::move(pending_dof);
  pending_dof = std::vector<int>();

  int l = 0;
  stopped_by_rows = false;
  while (l < p.max_levels - 1 && L[(size_t)l].A->global_rows() > p.max_coarse_size) {
    if (stop_rows > 0 && l >= 1 && L[(size_t)l].A->global_rows() <= stop_rows) {
      stopped_by_rows = true;  // the caller continues from here with a redundant hierarchy
      break;
    }
    LevelBuild b(l, L[(size_t)l], p, device_min_rows);
    b.begin("strength + coarsening");
    b.lap();
    level_same_function_operator(b);  // (charged to the strength phase)
    level_strength_and_coarsening(b);
    long long nc_glob = b.count_c_points();
    comm.allreduce_host(&nc_glob, 1, CommDType::I64, CommOp::SUM);
    if (nc_glob == 0 || nc_glob == b.A.global_rows() || nc_glob < p.min_coarse_size) break;

    b.begin("interpolation");
    b.lap();
    level_interpolation(b);
    if (!b.on_device) level_restriction(b);  // a host level's R is charged to the interpolation phase,
    t_phase[2] += b.lap();
    b.begin("Galerkin product");
    if (b.on_device) level_restriction(b);  // a device level's to the Galerkin phase, beside the products that read it
    level_galerkin_and_adopt(b);
    if (b.systems) L[(size_t)l + 1].dof = std::move(b.dof_coarse);
    l++;
  }
}

// l1 norms and the coarsest-level dense inverse, on the finished (C-first ordered, per-rank) levels
void BoomerAMG::finish_host() {
  Comm &comm = my_comm();
  // per-level norms (host), on the C-first ordered operators
  const int ch = chunk();
  for (size_t li = 0; li < L.size(); li++) {
    AmgLevel &Lv = L[li];
    ParCSR &A = *Lv.A;
    Lv.n = A.nrows;
    if (A.host_diag_stale && Lv.oA.nrows == A.nrows) {
      // the level lives on the device: norms straight into the solve-phase vectors
      hipStream_t s = ctx().stream;
      DVec<int> dcf_ext;
      Lv.d_diag.alloc((size_t)Lv.n);
      Lv.d_l1gs.alloc((size_t)Lv.n);
      Lv.d_l1jac.alloc((size_t)Lv.n);
      // N > 1 (levels of the distributed setup that were built on the device): the halo block's entries count too
      sk::DCsr dO;
      if (comm.size > 1) {
        std::vector<int> cf_ext;
        if (Lv.has_cf) cf_ext = A.halo_exchange_host_int(comm, Lv.cf.host());  // collective: gated by the global flag
        if (A.offd.nnz() > 0) {
          HostCSR O = A.offd;
          O.nrows = Lv.n;
          O.ncols = (int)A.col_map_offd.size();
          dO.upload(O, s);
          dcf_ext.upload(cf_ext);
        }
      }
      sk::level_norms(Lv.oA, Lv.cf.empty() ? nullptr : Lv.cf.dev(), ch, Lv.d_diag.p, Lv.d_l1gs.p, Lv.d_l1jac.p, s,
                      dO.nnz > 0 ? &dO : nullptr, dO.nnz > 0 ? dcf_ext.p : nullptr);
      MI_HIP(hipStreamSynchronize(s));
      continue;
    }
    std::vector<int> cf_ext;
    if (Lv.has_cf) cf_ext = A.halo_exchange_host_int(comm, Lv.cf.host());  // collective: gated by the global flag
    level_norms(A, Lv.cf.host(), cf_ext, ch, Lv.diag, Lv.l1gs, Lv.l1jac);
  }
  build_coarsest_inverse();
}

// coarsest level: dense inverse (relax type 9), every rank holds its own rows
void BoomerAMG::build_coarsest_inverse() {
  Comm &comm = my_comm();
  ensure_host((int)L.size() - 1);
  AmgLevel &Lc = L.back();
  const gidx ng = Lc.A->global_rows();
  if (!tail && p.relax_type[2] == 9 && ng <= MAX_DENSE && ng > 0) {
    ParCSR &A = *Lc.A;
    const int n = A.nrows;
    int maxloc = n;
    comm.allreduce_host(&maxloc, 1, CommDType::I32, CommOp::MAX);
    // gather all rows as (global row, global col, value) triples
    std::vector<char> mine;
    auto put = [&](gidx r, gidx c, double v) {
      const size_t off = mine.size();
      mine.resize(off + 2 * sizeof(gidx) + sizeof(double));
      memcpy(mine.data() + off, &r, sizeof(gidx));
      memcpy(mine.data() + off + sizeof(gidx), &c, sizeof(gidx));
      memcpy(mine.data() + off + 2 * sizeof(gidx), &v, sizeof(double));
    };
    for (int i = 0; i < n; i++) {
      for (int64_t k = A.diag.ia[(size_t)i]; k < A.diag.ia[(size_t)i + 1]; k++)
        put(A.row_start + i, A.row_start + A.diag.ja[(size_t)k], A.diag.a[(size_t)k]);
      for (int64_t k = A.offd.ia[(size_t)i]; k < A.offd.ia[(size_t)i + 1]; k++)
        put(A.row_start + i, A.col_map_offd[(size_t)A.offd.ja[(size_t)k]], A.offd.a[(size_t)k]);
    }
    std::vector<double> M((size_t)ng * ng, 0.0);
    auto absorb = [&](const std::vector<char> &buf) {
      const size_t rec = 2 * sizeof(gidx) + sizeof(double);
      for (size_t off = 0; off + rec <= buf.size(); off += rec) {
        gidx r, c;
        double v;
        memcpy(&r, buf.data() + off, sizeof(gidx));
        memcpy(&c, buf.data() + off + sizeof(gidx), sizeof(gidx));
        memcpy(&v, buf.data() + off + 2 * sizeof(gidx), sizeof(double));
        M[(size_t)r * ng + (size_t)c] = v;
      }
    };
    absorb(mine);
    if (comm.size > 1) {
      std::vector<int> peers;
      std::vector<std::vector<char>> send;
      for (int r = 0; r < comm.size; r++)
        if (r != comm.rank) {
          peers.push_back(r);
          send.push_back(mine);
        }
      std::vector<int> from;
      std::vector<std::vector<char>> got;
      comm.exchange_host(peers, send, from, got);
      for (auto &b : got) absorb(b);
    }
    std::vector<double> inv;
    dense_inverse((int)ng, M, inv);
    Lc.slot = maxloc;
    const size_t width = (size_t)comm.size * maxloc;
    std::vector<double> Mp((size_t)n * width, 0.0);
    for (int i = 0; i < n; i++)
      for (int r = 0; r < comm.size; r++) {
        const gidx rs = A.row_starts[(size_t)r], re = A.row_starts[(size_t)r + 1];
        for (gidx g = rs; g < re; g++)
          Mp[(size_t)i * width + (size_t)r * maxloc + (size_t)(g - rs)] = inv[(size_t)(A.row_start + i) * ng + (size_t)g];
      }
    Lc.Cinv_host.swap(Mp);
    Lc.dense = true;
  }
}

namespace {
// wrap a local CSR block as a (possibly rectangular) ParCSR without halo columns
std::unique_ptr<ParCSR> wrap_local(HostCSR &&M, const std::vector<gidx> &row_starts, const std::vector<gidx> &col_starts,
                                   int rank, bool device_resident = false) {
  std::unique_ptr<ParCSR> Q(new ParCSR());
  Q->nrows = M.nrows;
  Q->row_starts = row_starts;
  Q->col_starts = col_starts;
  Q->row_start = row_starts[(size_t)rank];
  Q->row_end = row_starts[(size_t)rank + 1];
  Q->offd.nrows = M.nrows;
  Q->offd.ncols = 0;
  if (!device_resident) Q->offd.ia.assign((size_t)M.nrows + 1, 0);  // (else: ParCSR::ensure_offd_rows)
  Q->diag = std::move(M);
  return Q;
}

// rows (given by their OLD global ids, in NEW order) of the global operator G, columns renumbered through
// colpos (global old -> global new) and split at this rank's column range into diag / halo blocks
std::unique_ptr<ParCSR> slice_rows(const HostCSR &G, const int *rows_old, int nloc, const int *colpos,
                                   const std::vector<gidx> &row_starts, const std::vector<gidx> &col_starts,
                                   int rank) {
  std::unique_ptr<ParCSR> Q(new ParCSR());
  const gidx c0 = col_starts[(size_t)rank], c1 = col_starts[(size_t)rank + 1];
  Q->nrows = nloc;
  Q->row_starts = row_starts;
  Q->col_starts = col_starts;
  Q->row_start = row_starts[(size_t)rank];
  Q->row_end = row_starts[(size_t)rank + 1];
  HostCSR &D = Q->diag, &O = Q->offd;
  D.nrows = O.nrows = nloc;
  D.ncols = (int)(c1 - c0);
  D.ia.assign((size_t)nloc + 1, 0);
  O.ia.assign((size_t)nloc + 1, 0);
  for (int q = 0; q < nloc; q++) {
    const int i = rows_old[q];
    int nd = 0;
    for (int64_t k = G.ia[(size_t)i]; k < G.ia[(size_t)i + 1]; k++) {
      const gidx c = colpos ? colpos[G.ja[(size_t)k]] : G.ja[(size_t)k];
      nd += (c >= c0 && c < c1);
    }
    D.ia[(size_t)q + 1] = D.ia[(size_t)q] + nd;
    O.ia[(size_t)q + 1] = O.ia[(size_t)q] + (G.ia[(size_t)i + 1] - G.ia[(size_t)i] - nd);
  }
  D.ja.resize((size_t)D.nnz());
  D.a.resize((size_t)D.nnz());
  O.ja.resize((size_t)O.nnz());
  O.a.resize((size_t)O.nnz());
  std::vector<gidx> ogid((size_t)O.nnz());
  parallel_for(nloc, [&](int64_t b, int64_t e, int) {
    std::vector<std::pair<gidx, double>> row;
    for (int64_t q = b; q < e; q++) {
      const int i = rows_old[q];
      row.clear();
      for (int64_t k = G.ia[(size_t)i]; k < G.ia[(size_t)i + 1]; k++)
        row.push_back({colpos ? (gidx)colpos[G.ja[(size_t)k]] : (gidx)G.ja[(size_t)k], G.a[(size_t)k]});
      std::sort(row.begin(), row.end(),
                [](const std::pair<gidx, double> &x, const std::pair<gidx, double> &y) { return x.first < y.first; });
      int64_t pd = D.ia[(size_t)q], po = O.ia[(size_t)q];
      for (auto &en : row) {
        if (en.first >= c0 && en.first < c1) {
          D.ja[(size_t)pd] = (int)(en.first - c0);
          D.a[(size_t)pd++] = en.second;
        } else {
          ogid[(size_t)po] = en.first;
          O.a[(size_t)po++] = en.second;
        }
      }
    }
  });
  Q->col_map_offd = ogid;
  std::sort(Q->col_map_offd.begin(), Q->col_map_offd.end());
  Q->col_map_offd.erase(std::unique(Q->col_map_offd.begin(), Q->col_map_offd.end()), Q->col_map_offd.end());
  for (size_t k = 0; k < ogid.size(); k++)
    O.ja[k] = (int)(std::lower_bound(Q->col_map_offd.begin(), Q->col_map_offd.end(), ogid[k]) - Q->col_map_offd.begin());
  O.ncols = (int)Q->col_map_offd.size();
  return Q;
}
}  // namespace

// single rank: the transfer operators have no halo block
void BoomerAMG::make_local_transfer_operators() {
  Comm &comm = my_comm();
  for (size_t l = 0; l + 1 < L.size(); l++) {
    AmgLevel &Lv = L[l];
    if (Lv.P.nrows == 0 && Lv.cf.empty()) continue;
    Lv.Pm = wrap_local(std::move(Lv.P), Lv.A->row_starts, L[l + 1].A->row_starts, comm.rank, Lv.oP.nrows > 0);
    Lv.Rm = wrap_local(std::move(Lv.R), L[l + 1].A->row_starts, Lv.A->row_starts, comm.rank, Lv.oP.nrows > 0);
    if (Lv.oP.nrows > 0) {  // built on the device: host arrays on demand
      Lv.Pm->host_diag_stale = Lv.Rm->host_diag_stale = true;
      Lv.Pm->dev_diag_nnz = Lv.oP.nnz;
      Lv.Rm->dev_diag_nnz = Lv.oR.nnz;
    }
    Lv.Pm->build_halo_plan(comm);
    Lv.Rm->build_halo_plan(comm);
    Lv.P = HostCSR();
    Lv.R = HostCSR();
  }
}

// More than one rank: coarsening, interpolation and the Galerkin products are
// GLOBAL algorithms, so the hierarchy -- and with it the
// iteration count -- does not depend on the number of ranks.  This first
// implementation obtains that by replication: every rank gathers the global
// operator, runs the single-rank setup on it and keeps its own rows of every
// level (in the per-rank C-first ordering) as distributed ParCSR blocks.  The
// solve phase is fully distributed; the setup is O(N_global) per rank and is
// the piece to distribute next.
void BoomerAMG::build_replicated(ParCSR &A0) {
  Comm &comm = my_comm();
  const int rank = comm.rank, size = comm.size;
  // ---- 1. gather the global operator (CSR over global columns)
  double tp0 = wall_time();
  const gidx N = A0.global_rows();
  MI_REQUIRE(N < (gidx)2147483000, "replicated setup: global row count exceeds int32");
  std::vector<char> mine;
  {
    const int n = A0.nrows;
    std::vector<int> len((size_t)n);
    size_t tot = 0;
    for (int i = 0; i < n; i++) {
      len[(size_t)i] = (int)((A0.diag.ia[(size_t)i + 1] - A0.diag.ia[(size_t)i]) +
                             (A0.offd.ia[(size_t)i + 1] - A0.offd.ia[(size_t)i]));
      tot += (size_t)len[(size_t)i];
    }
    // packed as [row lengths | columns | values]: the value section need not be 8-byte aligned, so the arrays are
    // filled on their own and copied in
    std::vector<int> cj(tot);
    std::vector<double> cv(tot);
    size_t q = 0;
    for (int i = 0; i < n; i++) {
      for (int64_t k = A0.diag.ia[(size_t)i]; k < A0.diag.ia[(size_t)i + 1]; k++, q++) {
        cj[q] = (int)(A0.row_start + A0.diag.ja[(size_t)k]);
        cv[q] = A0.diag.a[(size_t)k];
      }
      for (int64_t k = A0.offd.ia[(size_t)i]; k < A0.offd.ia[(size_t)i + 1]; k++, q++) {
        cj[q] = (int)A0.col_map_offd[(size_t)A0.offd.ja[(size_t)k]];
        cv[q] = A0.offd.a[(size_t)k];
      }
    }
    mine.resize(sizeof(int) * (size_t)n + tot * (sizeof(int) + sizeof(double)));
    char *w = mine.data();
    if (n) memcpy(w, len.data(), sizeof(int) * (size_t)n);
    if (tot) {
      memcpy(w + sizeof(int) * (size_t)n, cj.data(), tot * sizeof(int));
      memcpy(w + sizeof(int) * (size_t)n + tot * sizeof(int), cv.data(), tot * sizeof(double));
    }
  }
  std::vector<size_t> offs;
  std::vector<char> everyone;
  comm.allgatherv_host(mine.data(), mine.size(), offs, everyone);
  std::vector<char>().swap(mine);
  std::unique_ptr<ParCSR> Ag(new ParCSR());
  {
    HostCSR &G = Ag->diag;
    G.nrows = G.ncols = (int)N;
    G.ia.assign((size_t)N + 1, 0);
    std::vector<const char *> blob((size_t)size, nullptr);
    for (int r = 0; r < size; r++)
      if (offs[(size_t)r + 1] > offs[(size_t)r]) blob[(size_t)r] = everyone.data() + offs[(size_t)r];
    for (int r = 0; r < size; r++) {
      const gidx rs = A0.row_starts[(size_t)r], re = A0.row_starts[(size_t)r + 1];
      if (re > rs) MI_REQUIRE(blob[(size_t)r] != nullptr, "replicated setup: a rank's rows did not arrive");
      const int *len = reinterpret_cast<const int *>(blob[(size_t)r]);
      for (gidx g = rs; g < re; g++) G.ia[(size_t)g + 1] = G.ia[(size_t)g] + len[(size_t)(g - rs)];
    }
    G.ja.resize((size_t)G.nnz());
    G.a.resize((size_t)G.nnz());
    for (int r = 0; r < size; r++) {
      const gidx rs = A0.row_starts[(size_t)r], re = A0.row_starts[(size_t)r + 1];
      if (re == rs) continue;
      const size_t nr = (size_t)(re - rs);
      const size_t tot = (size_t)(G.ia[(size_t)re] - G.ia[(size_t)rs]);
      const char *base = blob[(size_t)r];
      memcpy(G.ja.data() + G.ia[(size_t)rs], base + sizeof(int) * nr, tot * sizeof(int));
      memcpy(G.a.data() + G.ia[(size_t)rs], base + sizeof(int) * nr + tot * sizeof(int), tot * sizeof(double));
    }
    // rows arrive as [diag | halo]: sort every row by global column
    parallel_for((int64_t)N, [&](int64_t b, int64_t e, int) {
      std::vector<std::pair<int, double>> row;
      for (int64_t i = b; i < e; i++) {
        const int64_t s0 = G.ia[(size_t)i], len = G.ia[(size_t)i + 1] - s0;
        bool sorted = true;
        for (int64_t k = 1; k < len; k++)
          if (G.ja[(size_t)(s0 + k)] < G.ja[(size_t)(s0 + k - 1)]) {
            sorted = false;
            break;
          }
        if (sorted) continue;
        row.resize((size_t)len);
        for (int64_t k = 0; k < len; k++) row[(size_t)k] = {G.ja[(size_t)(s0 + k)], G.a[(size_t)(s0 + k)]};
        std::sort(row.begin(), row.end(),
                  [](const std::pair<int, double> &x, const std::pair<int, double> &y) { return x.first < y.first; });
        for (int64_t k = 0; k < len; k++) {
          G.ja[(size_t)(s0 + k)] = row[(size_t)k].first;
          G.a[(size_t)(s0 + k)] = row[(size_t)k].second;
        }
      }
    });
    Ag->nrows = (int)N;
    Ag->row_start = 0;
    Ag->row_end = N;
    Ag->row_starts = {0, N};
    Ag->offd.nrows = (int)N;
    Ag->offd.ncols = 0;
    Ag->offd.ia.assign((size_t)N + 1, 0);
  }
  std::vector<char>().swap(everyone);
  const double t_gather = wall_time() - tp0;

  // ---- 2. the global hierarchy, natural ordering, through the single-rank code path
  BoomerAMG g;
  g.p = p;
  g.p.print_level = 0;
  g.device_min_rows = device_min_rows;
  g.keep_natural_R = true;
  g.stop_rows = effective_redundant_rows();
  g.use_private_self_comm();
  g.build_natural(*Ag);
  // a level below the threshold is redundant also when the coarsening ended on it (it is then the coarsest
  // level, and its smoother -- if it is not the dense solve -- must not stop at rank boundaries either)
  if (!g.stopped_by_rows && g.stop_rows > 0 && g.L.size() >= 2 && g.L.back().A->global_rows() <= g.stop_rows)
    g.stopped_by_rows = true;
  const bool has_tail = g.stopped_by_rows && g.L.size() >= 2;
  if (g.L[0].sA.ia.p && g.L[0].sA.nrows == (int)N) {  // level 0 lives on the device: drop the host copy
    HostCSR &G0 = Ag->diag;
    std::vector<int64_t>().swap(G0.ia);
    std::vector<int>().swap(G0.ja);
    std::vector<double>().swap(G0.a);
    Ag->host_diag_stale = true;
  }
  for (int q = 0; q < 4; q++) t_phase[q] = g.t_phase[q];
  tp0 = wall_time();
  const size_t nlev = g.L.size();

  // ---- 3. row partition of every level (coarse ownership = owner of the C point) and
  //         the per-rank C-first ordering: pos (old -> new), perm (new -> old), both global
  std::vector<std::vector<gidx>> starts(nlev);
  starts[0] = A0.row_starts;
  std::vector<std::vector<int>> pos(nlev), perm(nlev);
  for (size_t l = 0; l < nlev; l++) {
    const AmgLevel &G = g.L[l];
    const int n = G.A->nrows;
    if (l + 1 < nlev) {
      starts[l + 1].assign((size_t)size + 1, 0);
      for (int r = 0; r < size; r++) {
        gidx c = 0;
        for (gidx i = starts[l][(size_t)r]; i < starts[l][(size_t)r + 1]; i++) c += (G.cf[(size_t)i] == C_PT);
        starts[l + 1][(size_t)r + 1] = starts[l + 1][(size_t)r] + c;
      }
    }
    pos[l].resize((size_t)n);
    perm[l].resize((size_t)n);
    if (G.cf.empty()) {
      for (int i = 0; i < n; i++) pos[l][(size_t)i] = perm[l][(size_t)i] = i;
    } else {
      for (int r = 0; r < size; r++) {
        gidx q = starts[l][(size_t)r];
        for (gidx i = starts[l][(size_t)r]; i < starts[l][(size_t)r + 1]; i++)
          if (G.cf[(size_t)i] == C_PT) pos[l][(size_t)i] = (int)q++;
        for (gidx i = starts[l][(size_t)r]; i < starts[l][(size_t)r + 1]; i++)
          if (G.cf[(size_t)i] != C_PT) pos[l][(size_t)i] = (int)q++;
      }
      for (int i = 0; i < n; i++) perm[l][(size_t)pos[l][(size_t)i]] = i;
    }
  }

  // ---- 4. this rank's slices
  L.clear();
  L.resize(nlev);
  for (size_t l = 0; l < nlev; l++) {
    AmgLevel &G = g.L[l];
    AmgLevel &Lv = L[l];
    const gidx r0 = starts[l][(size_t)rank], r1 = starts[l][(size_t)rank + 1];
    const int nloc = (int)(r1 - r0);
    const int *rows_old = perm[l].data() + r0;
    hipStream_t s = ctx().stream;
    // a level the device built is sliced there (this rank's rows, columns renumbered, re-sorted) and only the
    // slice comes to the host; host-built levels are sliced from their host arrays
    auto slice = [&](sk::DCsr &dev, const HostCSR &host, bool host_ok, const int *rows, int nrows_loc,
                     const std::vector<int> &colpos, const std::vector<gidx> &rstarts,
                     const std::vector<gidx> &cstarts) -> std::unique_ptr<ParCSR> {
      if (dev.ia.p && dev.nnz > 0) {
        DVec<int> d_rows, d_pos;
        d_rows.upload(std::vector<int>(rows, rows + nrows_loc));
        d_pos.upload(colpos);
        sk::DCsr mine;
        sk::extract_rows(dev, d_rows.p, nrows_loc, d_pos.p, mine, s);
        HostCSR local;
        mine.download(local, s);
        std::vector<int> iota((size_t)nrows_loc);
        for (int q = 0; q < nrows_loc; q++) iota[(size_t)q] = q;
        return slice_rows(local, iota.data(), nrows_loc, nullptr, rstarts, cstarts, rank);
      }
      MI_REQUIRE(host_ok, "replicated setup: a level has neither device nor host arrays");
      return slice_rows(host, rows, nrows_loc, colpos.data(), rstarts, cstarts, rank);
    };
    Lv.A_own = slice(G.sA, G.A->diag, !G.A->host_diag_stale, rows_old, nloc, pos[l], starts[l], starts[l]);
    Lv.A = Lv.A_own.get();
    Lv.A->build_halo_plan(comm);
    Lv.has_cf = !G.cf.empty();
    if (Lv.has_cf) {
      const std::vector<int> &gcf = G.cf.host();
      std::vector<int> &lcf = Lv.cf.hostw(), &lperm = Lv.perm.hostw();
      lcf.resize((size_t)nloc);
      lperm.resize((size_t)nloc);
      Lv.nc = 0;
      for (int q = 0; q < nloc; q++) {
        lcf[(size_t)q] = gcf[(size_t)rows_old[q]];
        lperm[(size_t)q] = (int)(rows_old[q] - r0);
        Lv.nc += (lcf[(size_t)q] == C_PT);
      }
      // P: my fine rows x coarse columns; R = P^T: my coarse rows x fine columns
      Lv.Pm = slice(G.sP, G.P, !G.P.ia.empty(), rows_old, nloc, pos[l + 1], starts[l], starts[l + 1]);
      // with a redundant tail the coarse correction is whole on every rank: no exchange for the last P
      if (!(has_tail && l + 2 == nlev)) Lv.Pm->build_halo_plan(comm);
      const gidx c0 = starts[l + 1][(size_t)rank], c1 = starts[l + 1][(size_t)rank + 1];
      Lv.Rm = slice(G.sR, G.R, !G.R.ia.empty(), perm[l + 1].data() + c0, (int)(c1 - c0), pos[l], starts[l + 1], starts[l]);
      Lv.Rm->build_halo_plan(comm);
    }
    G.sP.release();
    G.sR.release();
    if (!(has_tail && l + 1 == nlev)) G.sA.release();
    // the global level is not needed any more (the tail's fine level is)
    if (has_tail && l + 1 == nlev && G.A_own)
      tail_A = std::move(G.A_own);
    else if (G.A_own)
      G.A_own.reset();
    G.P = HostCSR();
    G.R = HostCSR();
  }
  tail.reset();
  if (has_tail) {
    MI_REQUIRE(tail_A != nullptr, "replicated setup: the redundant level was not kept");
    // levels nlev-1 .. : one single-rank hierarchy per rank, built by the ordinary pipeline on the
    // (global, natural-order) operator of the first redundant level
    fetch_operator(tail_A.get(), g.L.back().sA);
    g.L.back().sA.release();
    tail.reset(new BoomerAMG());
    tail->p = p;
    tail->p.print_level = 0;
    tail->p.max_levels = std::max(1, p.max_levels - (int)(nlev - 1));
    tail->p.smooth_num_levels = std::max(0, p.smooth_num_levels - (int)(nlev - 1));
    tail->p.agg_num_levels = std::max(0, p.agg_num_levels - (int)(nlev - 1));
    tail->p.value_first_level = p.value_first_level - (int)(nlev - 1);
    tail->p.value_level_base = p.value_level_base + (int)(nlev - 1);
    tail->p.value_report = p.print_level > 0 && comm.rank == 0;
    {  // the tail counts its levels from 0: level-specific non-Galerkin tolerances move with it
      std::vector<double> shifted;
      for (size_t q = nlev - 1; q < p.non_galerkin_level_tol.size(); q++) shifted.push_back(p.non_galerkin_level_tol[q]);
      tail->p.non_galerkin_level_tol = shifted;
    }
    tail->device_min_rows = device_min_rows;
    tail->host_only = host_only;
    tail->use_private_self_comm();
    tail->setup_host(*tail_A);
    tail_start = starts[nlev - 1][(size_t)rank];
    int slot = 0;
    for (int r = 0; r < size; r++)
      slot = std::max(slot, (int)(starts[nlev - 1][(size_t)r + 1] - starts[nlev - 1][(size_t)r]));
    tail_slot = slot;
    std::vector<int> map((size_t)tail_A->nrows);
    for (int r = 0; r < size; r++)
      for (gidx i = starts[nlev - 1][(size_t)r]; i < starts[nlev - 1][(size_t)r + 1]; i++)
        map[(size_t)i] = r * slot + (int)(i - starts[nlev - 1][(size_t)r]);
    tail_map_host.swap(map);
  } else {
    tail_A.reset();
  }
  Ag.reset();
  t_phase[4] = wall_time() - tp0;
  if (p.print_level > 0 && rank == 0)
    printf("mi_hypre BoomerAMG: replicated setup on %d ranks (global gather %.2f s, slicing %.2f s)\n", size, t_gather,
           t_phase[4]);
}

// complex smoother (smooth_type 5 = ILU, 4 = FSAI) on levels < smooth_num_levels, never on the last level (which is the
// coarse solve, or the hand-over to the redundant tail): one block-Jacobi ILU(k) or FSAI of the level's diag block each
void BoomerAMG::build_smoothers() {
  Comm &comm = my_comm();
  for (size_t li = 0; li < L.size(); li++) {
    AmgLevel &Lv = L[li];
    Lv.smoother.reset();
    if ((p.smooth_type != 5 && p.smooth_type != 4) || (int)li >= p.smooth_num_levels || li + 1 >= L.size()) continue;
    if (p.smooth_type == 4) {
      auto fs = std::make_shared<FsaiSolver>();
      fs->algo_type = p.fsai_algo_type;
      fs->num_levels = p.fsai_num_levels;
      fs->threshold = p.fsai_threshold;
      fs->eig_max_iters = p.fsai_eig_max_iters;
      fs->max_steps = p.fsai_max_steps;
      fs->max_step_size = p.fsai_max_step_size;
      fs->kap_tolerance = p.fsai_kap_tolerance;
      fs->print_level = (p.print_level > 0 && comm.rank == 0) ? 1 : 0;
      fs->setup(*Lv.A, comm, "BoomerAMGSetup: level " + std::to_string(li));
      Lv.smoother = std::move(fs);
      continue;
    }
    ensure_host((int)li);
    auto ilu = std::make_shared<IluSolver>();
    ilu->ilu_type = p.ilu_type;
    ilu->level_of_fill = p.ilu_level;
    ilu->tri_solve = p.ilu_tri_solve;
    ilu->lower_it = p.ilu_lower_it;
    ilu->upper_it = p.ilu_upper_it;
    ilu->max_iter = p.ilu_max_iter;
    ilu->tol = 0.0;
    ilu->iter_type = p.ilu_iter_type;
    ilu->iter_option = p.ilu_iter_option;
    ilu->iter_max_iter = p.ilu_iter_max_iter;
    ilu->iter_tol = p.ilu_iter_tol;
    ilu->reordering = p.ilu_reordering;
    ilu->print_level = (p.print_level > 0 && comm.rank == 0) ? 1 : 0;
    ilu->setup(*Lv.A, comm);
    Lv.smoother = std::move(ilu);
  }
  fsai_signature = current_fsai_signature();
  for (AmgLevel &Lv : L) Lv.cheby = AmgLevel::Cheby();
  build_cheby();
}

namespace {
// number of eigenvalues below x of the symmetric tridiagonal matrix (d, e): sign changes of the Sturm sequence
int sturm_count(const std::vector<double> &d, const std::vector<double> &e, double x) {
  int count = 0;
  double q = 1.0;
  for (size_t i = 0; i < d.size(); i++) {
    const double off2 = i ? e[i - 1] * e[i - 1] : 0.0;
    if (q == 0.0) q = 1e-300;
    q = d[i] - x - off2 / q;
    if (q < 0.0) count++;
  }
  return count;
}
// smallest and largest eigenvalue of that matrix by bisection inside its Gershgorin interval
void tridiagonal_extremes(const std::vector<double> &d, const std::vector<double> &e, double &lmin, double &lmax) {
  const int m = (int)d.size();
  double gl = d[0], gu = d[0];
  for (int i = 0; i < m; i++) {
    const double r = (i ? std::fabs(e[(size_t)i - 1]) : 0.0) + (i + 1 < m ? std::fabs(e[(size_t)i]) : 0.0);
    gl = std::min(gl, d[(size_t)i] - r);
    gu = std::max(gu, d[(size_t)i] + r);
  }
  auto kth = [&](int k) {  // the k-th smallest (1-based): the supremum of { x : count(x) < k }
    double lo = gl, hi = gu;
    for (int it = 0; it < 2000; it++) {
      const double mid = lo + 0.5 * (hi - lo);
      if (!(mid > lo && mid < hi)) break;
      if (sturm_count(d, e, mid) >= k)
        hi = mid;
      else
        lo = mid;
    }
    return lo + 0.5 * (hi - lo);
  };
  lmin = kth(1);
  lmax = kth(m);
}
}  // namespace

std::vector<double> BoomerAMG::current_cheby_signature() const {
  if (!wants_cheby()) return {};
  return {(double)p.cheby_order, p.cheby_fraction, (double)p.cheby_eig_est, (double)p.cheby_variant, (double)p.cheby_scale};
}

void BoomerAMG::refresh_cheby() {
  if (cheby_signature != current_cheby_signature()) build_cheby();
}

// Chebyshev relaxation (relax type 16): per level the eigenvalue bounds of D^-1 A -- Gershgorin, or
// cheby_eig_est steps of conjugate gradients on D^-1/2 A D^-1/2 from the Park-Miller vector, whose coefficients give
// the Lanczos tridiagonal matrix -- then the interval, its centre and half width and the coefficients of the steps.
// Collective: every rank runs the same steps on every level (the stub in front of a redundant tail is never smoothed).
void BoomerAMG::build_cheby() {
  cheby_signature = current_cheby_signature();
  if (!wants_cheby()) return;
  if (p.cheby_order < 1 || p.cheby_order > 4 || !(p.cheby_fraction > 0.0 && p.cheby_fraction < 1.0) || p.cheby_eig_est < 0 ||
      p.cheby_variant != 0 || p.cheby_scale != 1) {
    for (AmgLevel &Lv : L) Lv.cheby.ready = false;
    fail(4, "BoomerAMG: Chebyshev order " + std::to_string(p.cheby_order) + ", fraction " + std::to_string(p.cheby_fraction) +
                ", eig_est " + std::to_string(p.cheby_eig_est) + ", variant " + std::to_string(p.cheby_variant) + ", scale " +
                std::to_string(p.cheby_scale) +
                " is not implemented (order 1 ... 4, fraction in (0, 1), eig_est >= 0, variant 0, scale 1 are); refusing to smooth "
                "with other settings");
  }
  Comm &comm = my_comm();
  hipStream_t s = ctx().stream;
  const size_t nlev = tail ? L.size() - 1 : L.size();
  for (size_t li = 0; li < nlev; li++) {
    AmgLevel &Lv = L[li];
    AmgLevel::Cheby &c = Lv.cheby;
    ParCSR &A = *Lv.A;
    const int n = Lv.n;
    const std::string where = "BoomerAMGSetup: level " + std::to_string(li) + ": Chebyshev relaxation (relax_type 16): ";
    if (!c.ready || c.eig_est != p.cheby_eig_est) {
      c.ready = false;
      DVec<double> w((size_t)n);
      double gmax = 0.0;
      long long bad = 0;
      k::gershgorin(A.d_diag, A.d_offd, Lv.d_diag.p, w.p, &gmax, &bad, s);
      double red[2] = {gmax, (double)bad};
      if (std::isnan(gmax)) red[0] = HUGE_VAL;  // (a maximum over the ranks that keeps a NaN visible)
      if (comm.size > 1) {
        comm.allreduce_host(&red[0], 1, CommDType::F64, CommOp::MAX);
        comm.allreduce_host(&red[1], 1, CommDType::F64, CommOp::SUM);
      }
      if (red[1] > 0.0)
        fail(4, where + std::to_string((long long)red[1]) +
                    " row(s) with a diagonal entry that is not positive: the smoother for such an operator is not "
                    "implemented (a positive diagonal is); refusing to smooth with something else");
      double emin = 0.0, emax = red[0];
      if (p.cheby_eig_est > 0) {
        DVec<double> dis((size_t)n), r((size_t)n), pv((size_t)n), t((size_t)n);
        k::inv_sqrt(Lv.d_diag.p, dis.p, n, s);
        sk::fsai_random_vector(n, (long long)A.row_start, 2747, r.p, s);
        k::copy(r.p, pv.p, n, s);
        double rr = par_dot_host(comm, r.p, r.p, n, s);
        std::vector<double> alpha, beta;
        for (int j = 0; j < p.cheby_eig_est; j++) {
          if (!(rr > 0.0)) break;  // the residual is zero
          k::vec_mul(pv.p, dis.p, t.p, n, s);
          A.matvec(comm, 1.0, t.p, 0.0, nullptr, w.p, s);
          k::vec_mul(w.p, dis.p, w.p, n, s);
          const double pBp = par_dot_host(comm, pv.p, w.p, n, s);
          if (!(pBp > 0.0)) break;
          const double al = rr / pBp;
          k::axpy(-al, w.p, r.p, n, s);
          const double rr_new = par_dot_host(comm, r.p, r.p, n, s);
          const double be = rr_new / rr;
          alpha.push_back(al);
          beta.push_back(be);
          rr = rr_new;
          k::scale(be, pv.p, n, s);
          k::axpy(1.0, r.p, pv.p, n, s);
        }
        MI_HIP(hipStreamSynchronize(s));  // the work vectors are released on leaving this block
        const size_t m = alpha.size();
        if (m == 0)
          fail(1, where + "the conjugate-gradient eigenvalue estimate made no step (zero start vector or p^T B p <= 0: the "
                          "operator is not positive definite)");
        std::vector<double> td(m), te(m > 1 ? m - 1 : 0);
        for (size_t j = 0; j < m; j++) {
          td[j] = 1.0 / alpha[j] + (j ? beta[j - 1] / alpha[j - 1] : 0.0);
          if (j + 1 < m) te[j] = std::sqrt(beta[j]) / alpha[j];
        }
        tridiagonal_extremes(td, te, emin, emax);
      }
      c.eig_min = emin;
      c.eig_max = emax;
      c.eig_est = p.cheby_eig_est;
    }
    c.upper = p.cheby_eig_est > 0 ? 1.1 * c.eig_max : c.eig_max;
    c.lower = c.eig_min + p.cheby_fraction * (c.upper - c.eig_min);
    c.theta = (c.upper + c.lower) / 2.0;
    c.delta = (c.upper - c.lower) / 2.0;
    if (!std::isfinite(c.eig_min) || !std::isfinite(c.upper) || !std::isfinite(c.lower) || !(c.upper > 0.0) || !(c.lower < c.upper)) {
      c.ready = false;
      fail(1, where + "eigenvalue bounds [" + std::to_string(c.lower) + ", " + std::to_string(c.upper) +
                  "] of D^-1 A are not a finite interval with a positive upper end");
    }
    c.order = p.cheby_order;
    const double sigma = c.theta / c.delta;
    double rho = 1.0 / sigma;
    c.a[0] = 0.0;
    c.b[0] = 1.0 / c.theta;
    for (int k = 1; k < c.order; k++) {
      const double rho_new = 1.0 / (2.0 * sigma - rho);
      c.a[k] = rho_new * rho;
      c.b[k] = 2.0 * rho_new / c.delta;
      rho = rho_new;
    }
    if (Lv.cheby_d.n != (size_t)n) Lv.cheby_d.alloc((size_t)n);
    c.ready = true;
  }
}

std::vector<double> BoomerAMG::current_fsai_signature() const {
  if (p.smooth_type == 5 && p.smooth_num_levels > 0 && p.ilu_iter_type != 0)
    return {(double)p.smooth_num_levels, (double)p.ilu_iter_type, (double)p.ilu_iter_option, (double)p.ilu_iter_max_iter,
            p.ilu_iter_tol};
  if (p.smooth_type != 4 || p.smooth_num_levels <= 0) return {};
  return {(double)p.smooth_num_levels, (double)p.fsai_algo_type, (double)p.fsai_num_levels, p.fsai_threshold,
          (double)p.fsai_eig_max_iters, (double)p.fsai_max_steps, (double)p.fsai_max_step_size, p.fsai_kap_tolerance};
}

// Value storage: the hierarchy is built as in mode 0; here, as the last step, the values of A, P
// and R of every level >= value_first_level are replaced by (double)(float)v -- in the host arrays that exist, in the
// halo blocks on the device (which keep 8-byte storage), and in the diag blocks on the device, which in mode 1 then
// hold floats only.  An operator with a finite non-zero value outside the normal floats' range, in either block on any
// rank, stays as it is: the ranks agree on the choice with one all-reduce, so it is that of a one-rank run.  The
// zero-guess sub-operators hold entries of A and follow A.
void BoomerAMG::apply_value_storage(bool on_device) {
  for (AmgLevel &Lv : L) Lv.value_kind[0] = Lv.value_kind[1] = Lv.value_kind[2] = 0;
  const int mode = p.value_storage;
  if (mode == 0) return;
  MI_REQUIRE(mode == 1 || mode == 2, "BoomerAMG: value storage mode must be 0, 1 or 2");
  Comm &comm = my_comm();
  hipStream_t s = on_device ? ctx().stream : nullptr;
  auto host_fits = [](const HostCSR &h) {
    for (double v : h.a)
      if (!k::fits_float(v)) return false;
    return true;
  };
  auto host_round = [](HostCSR &h) {
    for (double &v : h.a) v = (double)(float)v;
  };
  const size_t first = (size_t)std::max(0, p.value_first_level);
  auto operators = [](AmgLevel &Lv, ParCSR *ops[3]) { ops[0] = Lv.A, ops[1] = Lv.Pm.get(), ops[2] = Lv.Rm.get(); };
  // 1 where this rank's part of the operator fits; an operator that a rank does not hold counts as fitting there
  std::vector<int> fits(3 * L.size(), 1);
  for (size_t li = first; li < L.size(); li++) {
    ParCSR *ops[3];
    operators(L[li], ops);
    for (int op = 0; op < 3; op++) {
      ParCSR *M = ops[op];
      if (!M) continue;
      const bool placed = on_device && M->d_diag.ia.p != nullptr;
      MI_REQUIRE(!M->host_diag_stale || placed, "value storage: an operator has neither host nor device values");
      bool ok = host_fits(M->offd);
      if (!M->host_diag_stale)
        ok = ok && host_fits(M->diag);
      else
        ok = ok && k::values_fit_float(M->d_diag.a.p, M->d_diag.nnz, s);
      fits[3 * li + (size_t)op] = ok ? 1 : 0;
    }
  }
  if (comm.size > 1 && first < L.size()) comm.allreduce_host(fits.data() + 3 * first, 3 * (L.size() - first), CommDType::I32, CommOp::MIN);
  for (size_t li = first; li < L.size(); li++) {
    AmgLevel &Lv = L[li];
    ParCSR *ops[3];
    operators(Lv, ops);
    for (int op = 0; op < 3; op++) {
      ParCSR *M = ops[op];
      if (!M) continue;
      if (!fits[3 * li + (size_t)op]) {
        if ((p.print_level > 0 && comm.rank == 0) || p.value_report)
          printf("mi_hypre BoomerAMG: level %zu %s keeps fp64 values (a value outside the range of normal floats)\n",
                 li + (size_t)p.value_level_base, op == 0 ? "A" : op == 1 ? "P" : "R");
        continue;
      }
      const bool placed = on_device && M->d_diag.ia.p != nullptr;
      if (!M->host_diag_stale) host_round(M->diag);
      host_round(M->offd);
      if (placed) {
        k::narrow_values(M->d_diag, mode, s);
        if (M->d_diag.rowmap.p) ctx().n_value_row_mapped++;
        if (M->d_offd.a.p) k::round_values(M->d_offd.a.p, M->d_offd.nnz, s);
        if (op == 0 && Lv.has_Az) k::narrow_values(Lv.Az, mode, s);
        if (op == 0 && Lv.has_Ar) k::narrow_values(Lv.Ar, mode, s);
      }
      Lv.value_kind[op] = mode;
    }
  }
  if (on_device) MI_HIP(hipStreamSynchronize(s));
}

void BoomerAMG::setup_device() {
  TraceRange trace_setup("mi_hypre BoomerAMGSetup (solve-phase format)");
  MI_REQUIRE(host_ready, "BoomerAMG: setup_device before setup_host");
  ensure_init();
  Comm &comm = my_comm();
  const int ch = chunk();
  const bool timing = getenv("MI_HYPRE_SETUP_TIMING") != nullptr && comm.rank == 0;
  for (size_t li = 0; li < L.size(); li++) {
    AmgLevel &Lv = L[li];
    hipStream_t s = ctx().stream;
    const double tdev0 = wall_time();
    struct LevelTimer {
      bool on;
      size_t l;
      double t0;
      ~LevelTimer() {
        if (on) {
          (void)hipDeviceSynchronize();
          printf("   solve-phase format: level %zu %.2f s\n", l, wall_time() - t0);
        }
      }
    } level_timer{timing && li < 4, li, tdev0};
    const std::string fname = "format: level " + std::to_string(li) + " ";
    std::unique_ptr<TraceRange> trace_f(new TraceRange((fname + "A").c_str()));
    auto place = [&](ParCSR &M, sk::DCsr &dev) {
      if (dev.nrows == M.nrows && M.host_diag_stale) {  // built on the device: no host round trip
        sk::to_solve_format(dev, M.d_diag, s);
        M.to_device_halo();
      } else {
        M.to_device();
      }
    };
    if (li > 0 || !Lv.A->on_device) place(*Lv.A, Lv.oA);
    // transfer operators are SpMV-only and short-rowed: more rows per tile (MI_HYPRE_SPMV_ROW_CAP, in rows)
    static const int spmv_cap = getenv("MI_HYPRE_SPMV_ROW_CAP") ? atoi(getenv("MI_HYPRE_SPMV_ROW_CAP")) : k::SPMV_ONLY_ROW_CAP;
    if (Lv.Pm) Lv.Pm->d_diag.row_cap = spmv_cap;
    if (Lv.Rm) Lv.Rm->d_diag.row_cap = spmv_cap;
    trace_f.reset(), trace_f.reset(new TraceRange((fname + "P").c_str()));
    if (Lv.Pm) place(*Lv.Pm, Lv.oP);
    trace_f.reset(), trace_f.reset(new TraceRange((fname + "R").c_str()));
    // Restriction: the coarse vectors live in the coarse level's C-first order, in which neighbouring rows of R are
    // NOT neighbouring coarse points of the fine level (first the coarse level's C points, then its F points): a
    // tile of R then gathers a thinned-out stretch of the fine vector, and every line of it is fetched by several
    // tiles (4x the vector's bytes at 512^3).  R is therefore stored with its rows in the order the coarse points
    // have on the FINE level (= the coarse level's ordering before its own C-first step) and writes through a row map.
    const bool r_on_device = Lv.Rm && Lv.oR.nrows == Lv.Rm->nrows && Lv.Rm->host_diag_stale;  // built there
    static const long long nat_min = getenv("MI_HYPRE_NATURAL_R_MIN_NNZ") ? atoll(getenv("MI_HYPRE_NATURAL_R_MIN_NNZ")) : 4000000;
    const bool r_large_host = Lv.Rm && !Lv.Rm->host_diag_stale && Lv.Rm->diag.nnz() >= nat_min;  // e.g. distributed setup
    if (Lv.Rm && li + 1 < L.size() && (r_on_device || r_large_host) &&
        L[li + 1].perm.size() == (size_t)Lv.Rm->nrows && Lv.Rm->nrows > 0) {
      // L[li + 1].perm: stored position -> position before the C-first step; its inverse orders the rows of R
      DVec<int> dpos(L[li + 1].perm.size());
      sk::invert_permutation(L[li + 1].perm.dev(), (int)L[li + 1].perm.size(), dpos.p, s);
      sk::DCsr nat;
      if (r_on_device) {
        sk::permute(Lv.oR, dpos.p, nullptr, nat, s);
        Lv.oR.release();
      } else {
        sk::DCsr raw;
        raw.upload(Lv.Rm->diag, s);
        sk::permute(raw, dpos.p, nullptr, nat, s);
      }
      sk::to_solve_format(nat, Lv.Rm->d_diag, s);
      Lv.Rm->d_diag.rowmap = std::move(dpos);
      Lv.Rm->to_device_halo();
    } else if (Lv.Rm) {
      Lv.Rm->d_diag.rowmap.release();
      place(*Lv.Rm, Lv.oR);
    }
    // the down leg starts every level from u = 0: its sweep runs on the entries that can see non-zeros
    trace_f.reset(), trace_f.reset(new TraceRange((fname + "zero-guess sub-operators").c_str()));
    Lv.has_Az = false;
    Lv.Az = DevCSR();
    const int t0 = p.relax_type[0];
    const bool down_gs = t0 == 3 || t0 == 4 || t0 == 6 || t0 == 8 || t0 == 13 || t0 == 14;  // hybrid GS family
    if (zero_skip_mode() > 1 && down_gs && Lv.has_cf && !Lv.cf.empty() && Lv.n > 0 && Lv.nc > 0 &&
        Lv.A->d_diag.nrows == Lv.n && Lv.A->d_diag.ncols == Lv.n) {
      sk::DCsr Z;
      sk::zero_guess_operator(Lv.A->d_diag, Lv.nc, ch, Z, s);
      sk::to_solve_format(Z, Lv.Az, s);
      Lv.has_Az = true;
      Lv.Az_chunk = ch;
      Lv.has_Ar = false;
      Lv.Ar = DevCSR();
      Lv.t_valid = false;
      if (zero_skip_mode() > 2 && ch == 8 && li + 1 < L.size()) {  // a residual follows the down sweep
        sk::DCsr R;
        sk::zero_guess_operator(Lv.A->d_diag, Lv.nc, ch, R, s, 1);
        Lv.Ar.row_cap = spmv_cap;
        sk::to_solve_format(R, Lv.Ar, s);
        Lv.t_from = (Lv.nc + ch - 1) / ch * ch;
        Lv.tvec.alloc((size_t)Lv.n);
        zero_on_stream(Lv.tvec.p, (size_t)Lv.n * sizeof(double));
        Lv.has_Ar = true;
        Lv.Az.prefer_gs_tiles = true;  // only the tile kernel hands the F pass's C-column product over
      }
    }
    // C-row hand-over: the tiles of level 0 the Krylov mat-vec still runs after the cycle's last C pass
    Lv.mv_tdesc.release();
    Lv.handover = sk::HandoverCensus();
    if (li == 0 && !forced_comm && comm.size == 1 && ch == 8 && Lv.has_cf && !Lv.cf.empty() && Lv.nc > 0 && Lv.nc < Lv.n &&
        Lv.A->d_diag.nrows == Lv.n && Lv.A->d_diag.ncols == Lv.n && k::gs_uses_tiles(Lv.A->d_diag, ch))
      sk::handover_tiles(Lv.A->d_diag, Lv.nc, Lv.mv_tdesc, Lv.handover, s);
    trace_f.reset(), trace_f.reset(new TraceRange((fname + "vectors, C/F marks, permutation").c_str()));
    if (!Lv.d_diag.p || Lv.d_diag.n != (size_t)Lv.n) {
      Lv.d_diag.upload(Lv.diag);
      Lv.d_l1gs.upload(Lv.l1gs);
      Lv.d_l1jac.upload(Lv.l1jac);
    }
    if (!Lv.cf.empty()) {
      Lv.d_cf.alloc(Lv.cf.size());
      sk::ints_to_i8(Lv.cf.dev(), (long long)Lv.cf.size(), Lv.d_cf.p, s);
    }
    if (!Lv.perm.empty()) {
      Lv.d_perm.alloc(Lv.perm.size());
      MI_HIP(hipMemcpyAsync(Lv.d_perm.p, Lv.perm.dev(), Lv.perm.size() * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    Lv.mv = AmgLevel::MvVectors();  // the next batched cycle allocates its vectors again
    Lv.u.alloc((size_t)Lv.n);
    Lv.f.alloc((size_t)Lv.n);
    Lv.tmp.alloc((size_t)Lv.n);
    Lv.snap.alloc((size_t)Lv.n);
    if (Lv.n) {
      zero_on_stream(Lv.u.p, (size_t)Lv.n * sizeof(double));
      zero_on_stream(Lv.f.p, (size_t)Lv.n * sizeof(double));
      zero_on_stream(Lv.tmp.p, (size_t)Lv.n * sizeof(double));
      zero_on_stream(Lv.snap.p, (size_t)Lv.n * sizeof(double));
    }
  }
  build_smoothers();
  apply_value_storage(true);  // after everything Setup derives from the operators as built
  upload_coarsest_inverse();
  if (tail) {
    tail->setup_device();
    const size_t ng = (size_t)tail_A->nrows;
    tail_fslot.alloc((size_t)tail_slot);
    tail_fgather.alloc((size_t)tail_slot * (size_t)comm.size);
    tail_f.alloc(ng);
    tail_e.alloc(ng);
    zero_on_stream(tail_fslot.p, ((size_t)tail_slot + 2) * sizeof(double));
    zero_on_stream(tail_fgather.p, ((size_t)tail_slot * (size_t)comm.size + 2) * sizeof(double));
    zero_on_stream(tail_e.p, (ng + 2) * sizeof(double));
    tail_map.upload(tail_map_host);
    AmgLevel &Lp = L[L.size() - 2];
    std::vector<int> pcol(Lp.Pm->col_map_offd.size());
    for (size_t q = 0; q < pcol.size(); q++) pcol[q] = (int)Lp.Pm->col_map_offd[q];
    tail_pcol.upload(pcol);
  }
  MI_HIP(hipDeviceSynchronize());
  sk::release_host_scratch();
  dev_pool_trim();  // the setup's transient buffers go back to the driver: the solve allocates its Krylov basis next
  {
    TraceRange tr("format: collapsed coarse tail");
    const double tc0 = wall_time();
    build_collapsed_tail();
    if (timing && collapsed_level >= 0)
      printf("   collapsed coarse tail: levels %d.. as one %d x %d map, %.3f s\n", collapsed_level, collapsed_n, collapsed_n,
             wall_time() - tc0);
  }
  is_setup = true;
  setup_seconds = wall_time() - t_setup_start;
  if (timing) {
    long long mp = 0, iu = 0, pm = 0, pu = 0, gr = 0, dr = 0;
    double tg = 0.0, td = 0.0, tw = 0.0;
    dev_arena_stats(&mp, &iu, &pm, &pu);
    dev_arena_times(&tg, &td, &gr, &dr, &tw);
    printf("   device arena (since the process started): %.1f GiB mapped (peak %.1f), %.1f GiB in use (peak %.1f); %lld chunks mapped, %.2f s inside "
           "hipMemCreate/Map (grow-ahead thread), requests waited %.2f s for it; %lld stream drains before a reuse, %.2f s\n",
           mp / 1073741824.0, pm / 1073741824.0, iu / 1073741824.0, pu / 1073741824.0, gr, tg, tw, dr, td);
    printf("   value dictionaries (1-byte value stream):");
    for (size_t li = 0; li < L.size(); li++) {
      const AmgLevel &Lv = L[li];
      auto dict = [](const DevCSR &D) { return D.value_format() == ValueFormat::DICT; };
      printf(" L%zu[%s%s%s%s%s]", li, dict(Lv.A->d_diag) ? "A" : "", Lv.has_Az && dict(Lv.Az) ? " Az" : "",
             Lv.has_Ar && dict(Lv.Ar) ? " Ar" : "", Lv.Pm && dict(Lv.Pm->d_diag) ? " P" : "", Lv.Rm && dict(Lv.Rm->d_diag) ? " R" : "");
    }
    printf("\n");
  }
  if (p.print_level > 0 && comm.rank == 0) {
    printf("mi_hypre BoomerAMG setup: %d levels, operator complexity %.3f, chunk %d, %.3f s\n", total_levels(),
           operator_complexity(), ch, setup_seconds);
    printf("   hierarchy build, wall per phase: strength %.2f  pmis %.2f  interp %.2f  galerkin %.2f  C-first ordering %.2f  (total %.2f) s\n",
           t_phase[0], t_phase[1], t_phase[2], t_phase[3], t_phase[4], t_phase[5]);
    for (int li = 0; li < total_levels(); li++) {
      int loc = 0;
      BoomerAMG &o = owner_of(li, loc);
      const AmgLevel &Lv = o.L[(size_t)loc];
      std::string per_function;  // num_functions > 1: the level's rows by the unknown they belong to
      if (p.num_functions > 1 && Lv.dof.size() == (size_t)Lv.n) {
        std::vector<long long> rows((size_t)p.num_functions, 0);
        for (int d : Lv.dof.host()) rows[(size_t)d]++;
        per_function = "  rows per function";
        for (size_t f = 0; f < rows.size(); f++) per_function += (f ? " / " : " ") + std::to_string(rows[f]);
      }
      printf("   level %2d: local rows %10d  global rows %12lld  local nnz %12lld%s%s\n", li, Lv.n,
             (long long)Lv.A->global_rows(), (long long)(Lv.A->diag_nnz() + Lv.A->offd.nnz()),
             &o != this ? "  (whole level on every rank)" : "", per_function.c_str());
    }
  }
}

void BoomerAMG::upload_coarsest_inverse() {
  AmgLevel &Lc = L.back();
  if (!Lc.dense) return;
  const size_t width = (size_t)my_comm().size * (size_t)Lc.slot;
  if (Lc.Cinv.p && Lc.Cinv.n == Lc.Cinv_host.size() && Lc.fgather.n == width && Lc.fslot.n == (size_t)Lc.slot) {
    // a refresh: the buffers of the build take the new inverse (the gather buffers hold nothing between cycles)
    if (!Lc.Cinv_host.empty()) Lc.Cinv.upload(Lc.Cinv_host.data(), Lc.Cinv_host.size());
    return;
  }
  Lc.Cinv.upload(Lc.Cinv_host);
  Lc.fgather.alloc(width);
  Lc.fslot.alloc((size_t)Lc.slot);
  zero_on_stream(Lc.fslot.p, ((size_t)Lc.slot + 2) * sizeof(double));
  zero_on_stream(Lc.fgather.p, (width + 2) * sizeof(double));
}

// ------------------------------------------------------------------ setup reuse ("Setup reuse")
namespace {
long long g_setups_full = 0, g_setups_refreshed = 0;
const char *const REBUILD_REASON[7] = {"reuse is off",
                                       "first Setup of this handle, or the previous one failed",
                                       "another matrix object or another pattern",
                                       "a setting the structure depends on changed since the last Setup",
                                       "a setting the refresh does not cover is on (non-Galerkin tolerances, value storage, restriction 1, "
                                       "one-point interpolation or num_functions > 1)",
                                       "more than one rank",
                                       "the other setup entry point built the hierarchy"};
}  // namespace

const char *setup_reuse_reason_text(int reason) { return reason >= 0 && reason < 7 ? REBUILD_REASON[reason] : "unknown reason"; }

long long setup_reuse_counter(const char *name) {
  const std::string n(name ? name : "");
  return n == "amg_setups_full" ? g_setups_full : n == "amg_setups_refreshed" ? g_setups_refreshed : -1;
}

// Everything the kept part of a hierarchy depends on: the splittings and P (coarsening, interpolation, truncation, level
// limits, aggressive settings), the orderings (locality numbering), the sub-operators' patterns (GS chunk, zero-guess
// mode, whether the down smoother is of the Gauss-Seidel family), what exists besides (coarsest dense inverse, value
// dictionaries, value storage, non-Galerkin sparsification) and which levels the device built.
std::vector<double> BoomerAMG::current_structure_signature(const ParCSR &A) const {
  std::vector<double> v = {(double)p.coarsen_type, (double)p.interp_type, p.strong_threshold, p.max_row_sum, p.trunc_factor,
                           (double)p.pmax_elmts, (double)p.max_levels, (double)p.max_coarse_size, (double)p.min_coarse_size,
                           (double)p.agg_num_levels, (double)p.agg_interp_type, (double)p.agg_pmax_elmts, p.agg_trunc_factor,
                           (double)p.agg_p12_max_elmts, p.agg_p12_trunc_factor, (double)p.keep_agg_markers,
                           use_locality_order(A) ? 1.0 : 0.0, (double)chunk(), (double)zero_skip_mode(),
                           k::value_dictionary_enabled() ? 1.0 : 0.0, (double)p.value_storage, (double)p.value_first_level,
                           p.non_galerkin_tol, (double)p.restriction, p.strong_threshold_r, p.filter_threshold_r};
  for (double t : p.non_galerkin_level_tol) v.push_back(t);
  const int t0 = p.relax_type[0];
  v.push_back((t0 == 3 || t0 == 4 || t0 == 6 || t0 == 8 || t0 == 13 || t0 == 14) ? 1.0 : 0.0);
  v.push_back(p.relax_type[2] == 9 ? 1.0 : 0.0);
  v.push_back((double)default_device_min_rows());
  v.push_back((double)p.num_functions);
  v.push_back(wants_mcgs() ? 1.0 : 0.0);  // (the levels are coloured and ordered by colour: relax types 40 / 41 / 42)
  return v;
}

int BoomerAMG::refresh_verdict(const ParCSR &A, bool entry_host_only) const {
  if (setup_reuse == 0) return 0;
  if (!built_ok || L.empty()) return 1;
  if (my_comm().size > 1) return 5;
  if (built_host_only != entry_host_only) return 6;
  if (built_matrix != &A || built_pattern != A.pattern_stamp) return 2;
  if (p.non_galerkin() || p.value_storage != 0) return 4;
  // (the neighbourhoods and the filter of an approximate ideal restriction and the choice of one-point interpolation
  // depend on the values: their patterns are not kept)
  if (p.restriction != 0 || p.interp_type == 100) return 4;
  if (p.num_functions > 1) return 4;  // (the refresh has no same-function operator, and dof_func may have changed)
  if (structure_signature != current_structure_signature(A)) return 3;
  return -1;
}

void BoomerAMG::build_from_scratch(ParCSR &A, bool entry_host_only) {
  host_only = entry_host_only;
  if (entry_host_only) {
    device_min_rows = -1;  // host threads only
    setup_host(A);
    apply_value_storage(false);
    if (tail) tail->apply_value_storage(false);
  } else {
    device_min_rows = default_device_min_rows();
    setup_host(A);
    setup_device();
  }
}

void BoomerAMG::setup_entry(ParCSR &A, bool entry_host_only) {
  const int verdict = refresh_verdict(A, entry_host_only);
  built_ok = false;  // a Setup that fails leaves the handle not set up: the next one rebuilds (reason 1)
  if (verdict < 0) {
    is_setup = false;
    host_ready = false;
    host_only = entry_host_only;
    validate_settings();  // cycle settings may have changed since the build: what a full Setup refuses is refused here too
    refresh(A);
    setup_kind = 2, setup_reason = 0;
    g_setups_refreshed++;
  } else {
    build_from_scratch(A, entry_host_only);
    setup_kind = 1, setup_reason = verdict;
    g_setups_full++;
    built_host_only = entry_host_only;
    built_matrix = &A;
    built_pattern = A.pattern_stamp;
    structure_signature = current_structure_signature(A);
  }
  built_ok = true;
  if (!entry_host_only) {
    source_matrix = &A;
    source_stamp = A.assembly_stamp;
  }
  if (p.print_level > 0 && my_comm().rank == 0 && setup_reuse != 0) {
    if (setup_kind == 2)
      printf("mi_hypre BoomerAMG setup: refreshed (values on the kept structure), %.3f s\n", setup_seconds);
    else
      printf("mi_hypre BoomerAMG setup: rebuilt from scratch: %s\n", REBUILD_REASON[setup_reason]);
  }
}

namespace {
// stored entry (r, c) of D takes the caller's entry (perm[r], perm[c]); false (and the row) when the caller has none
bool host_value_lookup(HostCSR &D, const std::vector<int> &perm, const HostCSR &S, int &bad_row) {
  std::vector<double> a((size_t)D.nnz());
  std::atomic<int> bad{INT_MAX};
  parallel_for(D.nrows, [&](int64_t b, int64_t e, int) {
    for (int64_t r = b; r < e; r++) {
      const int sr = perm[(size_t)r];
      const int *s0 = S.ja.data() + S.ia[(size_t)sr], *s1 = S.ja.data() + S.ia[(size_t)sr + 1];
      for (int64_t k = D.ia[(size_t)r]; k < D.ia[(size_t)r + 1]; k++) {
        const int sc = perm[(size_t)D.ja[(size_t)k]];
        const int *q = std::lower_bound(s0, s1, sc);
        if (q == s1 || *q != sc) {
          int cur = bad.load();
          while ((int)r < cur && !bad.compare_exchange_weak(cur, (int)r)) {
          }
          continue;
        }
        a[(size_t)k] = S.a[(size_t)(q - S.ja.data())];
      }
    }
  });
  bad_row = bad.load();
  if (bad_row != INT_MAX) return false;
  D.a.swap(a);
  return true;
}

void values_to_host(const DevCSR &D, HostCSR &H, hipStream_t s) {
  MI_REQUIRE((int64_t)H.a.size() == D.nnz, "setup reuse: host and device copies of an operator differ in size");
  if (D.nnz) d2h(H.a.data(), D.a.p, (size_t)D.nnz * sizeof(double), s);
}
}  // namespace

// step 1: the hierarchy's own copy of the caller's matrix (internal numbering, then C-first) takes the new values
void BoomerAMG::refresh_level0(ParCSR &A0) {
  AmgLevel &L0 = L[0];
  if (L0.A == &A0) return;  // no copy: level 0 is the caller's matrix itself
  ParCSR &A = *L0.A;
  MI_REQUIRE(L0.perm.size() == (size_t)A0.nrows && A.nrows == A0.nrows, "setup reuse: level 0 has no permutation of the caller's rows");
  const std::string where = "BoomerAMGSetup (refresh): level 0: internal error: the caller's matrix has no entry for a stored one (row ";
  if (!host_only && A0.on_device && A0.d_diag.a.p) {
    hipStream_t s = ctx().stream;
    const int bad = sk::value_lookup(A.d_diag, L0.d_perm.p, L0.d_perm.p, A0.d_diag, s);
    if (bad >= 0) fail(1, where + std::to_string(bad) + ")");
    if (!A.host_diag_stale) values_to_host(A.d_diag, A.diag, s);
  } else {
    if (!host_only) ensure_host(0);
    int bad = 0;
    if (!host_value_lookup(A.diag, L0.perm.host(), A0.diag, bad)) fail(1, where + std::to_string(bad) + ")");
    if (!host_only && A.d_diag.nnz)
      MI_HIP(hipMemcpy(A.d_diag.a.p, A.diag.a.data(), (size_t)A.d_diag.nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!host_only) k::build_value_dictionary(A.d_diag, ctx().stream);  // the value format is decided again
}

// step 2: A_{level+1} = P^T (A P) into its stored pattern, in the order contract of host_spgemm on the stored operators
void BoomerAMG::refresh_coarse_operator(int level, double *seconds) {
  AmgLevel &Lf = L[(size_t)level], &Lc = L[(size_t)level + 1];
  const std::string where = "BoomerAMGSetup (refresh): level " + std::to_string(level + 1) + ": internal error: ";
  if (!Lf.Pm || !Lf.Rm) fail(1, where + "the level above has no transfer operators");
  ParCSR &C = *Lc.A;
  if (!host_only) {
    hipStream_t s = ctx().stream;
    const int bad = sk::galerkin_values(Lf.A->d_diag, Lf.Pm->d_diag, Lf.Rm->d_diag, C.d_diag, s, seconds);
    if (bad >= 0) fail(1, where + "the Galerkin product's pattern is not the stored one (row " + std::to_string(bad) + ")");
    k::build_value_dictionary(C.d_diag, s);
    if (!C.host_diag_stale) values_to_host(C.d_diag, C.diag, s);
    return;
  }
  const double t0 = wall_time();
  HostCSR T, G;
  host_spgemm(Lf.A->diag, Lf.Pm->diag, T);
  const double t1 = wall_time();
  host_spgemm(Lf.Rm->diag, T, G);
  if (G.nrows != C.diag.nrows || G.ia != C.diag.ia || G.ja != C.diag.ja)
    fail(1, where + "the Galerkin product's pattern is not the stored one");
  C.diag.a.swap(G.a);
  if (seconds) seconds[0] = t1 - t0, seconds[1] = wall_time() - t1;
}

// step 3: diagonal and l1 norms, and the values of the zero-guess sub-operators (entry subsets of A on kept patterns)
void BoomerAMG::refresh_norms_and_sub_operators(int level) {
  AmgLevel &Lv = L[(size_t)level];
  ParCSR &A = *Lv.A;
  const int ch = chunk();
  Lv.t_valid = false;
  if (host_only) {
    level_norms(A, Lv.cf.host(), {}, ch, Lv.diag, Lv.l1gs, Lv.l1jac);
    return;
  }
  hipStream_t s = ctx().stream;
  if (Lv.n) {
    sk::level_norms(A.d_diag, Lv.cf.empty() ? nullptr : Lv.cf.dev(), ch, Lv.d_diag.p, Lv.d_l1gs.p, Lv.d_l1jac.p, s);
    if (!Lv.diag.empty()) {  // a level the host built keeps its host copies
      d2h(Lv.diag.data(), Lv.d_diag.p, (size_t)Lv.n * sizeof(double), s);
      d2h(Lv.l1gs.data(), Lv.d_l1gs.p, (size_t)Lv.n * sizeof(double), s);
      d2h(Lv.l1jac.data(), Lv.d_l1jac.p, (size_t)Lv.n * sizeof(double), s);
    }
  }
  const std::string where = "BoomerAMGSetup (refresh): level " + std::to_string(level) + ": internal error: ";
  if (Lv.has_Az) {
    const int bad = sk::value_lookup(Lv.Az, nullptr, nullptr, A.d_diag, s);
    if (bad >= 0) fail(1, where + "the zero-guess sub-operator has an entry the operator lacks (row " + std::to_string(bad) + ")");
    k::build_value_dictionary(Lv.Az, s);
  }
  if (Lv.has_Ar) {
    const int bad = sk::value_lookup(Lv.Ar, nullptr, nullptr, A.d_diag, s);
    if (bad >= 0) fail(1, where + "the residual sub-operator has an entry the operator lacks (row " + std::to_string(bad) + ")");
    k::build_value_dictionary(Lv.Ar, s);
  }
}

// A Setup that keeps the structure (cf, both permutations, nc, P, R, every pattern, tile schedule and column list, the
// work vectors) and recomputes what depends on the values, level by level.  One rank.
void BoomerAMG::refresh(ParCSR &A0) {
  TraceRange trace_setup("mi_hypre BoomerAMGSetup (refresh)");
  const bool timing = getenv("MI_HYPRE_SETUP_TIMING") != nullptr;
  t_setup_start = wall_time();
  for (double &t : t_phase) t = 0.0;
  double t0 = wall_time();
  refresh_level0(A0);
  if (timing) printf("   refresh: level-0 values %.3f s\n", wall_time() - t0);
  for (int l = 0; l + 1 < (int)L.size(); l++) {
    double sec[2] = {0.0, 0.0};
    t0 = wall_time();
    refresh_coarse_operator(l, sec);
    t_phase[3] += wall_time() - t0;
    if (timing && l < 4) printf("   refresh: level %d Galerkin values %.3f s (A P %.3f, P^T T into the pattern %.3f)\n", l + 1, wall_time() - t0, sec[0], sec[1]);
  }
  if (timing) printf("   refresh: Galerkin values, all levels %.3f s\n", t_phase[3]);
  t0 = wall_time();
  for (int l = 0; l < (int)L.size(); l++) refresh_norms_and_sub_operators(l);
  build_coarsest_inverse();
  host_ready = true;
  if (timing) printf("   refresh: norms, sub-operators, coarsest inverse %.3f s\n", wall_time() - t0);
  if (!host_only) {
    t0 = wall_time();
    upload_coarsest_inverse();
    build_smoothers();
    MI_HIP(hipDeviceSynchronize());
    if (timing) printf("   refresh: smoothers %.3f s\n", wall_time() - t0);
    t0 = wall_time();
    build_collapsed_tail();
    if (timing) printf("   refresh: collapsed tail %.3f s\n", wall_time() - t0);
    is_setup = true;
  }
  t_phase[5] = wall_time() - t_setup_start;
  setup_seconds = t_phase[5];
  if (timing && !host_only) {
    long long mp = 0, iu = 0, pm = 0, pu = 0;
    dev_arena_stats(&mp, &iu, &pm, &pu);
    printf("   refresh: total %.3f s; device arena %.1f GiB in use (peak %.1f)\n", setup_seconds, iu / 1073741824.0, pu / 1073741824.0);
  }
}

}  // namespace mi
