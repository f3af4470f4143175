// Distributed BoomerAMG setup on N > 1 ranks (SURVEY.md 8e "coarse levels inherit the partition", 8 f2;
// partition rule: init_row_decomposition, /root/reference/src/HypreSystem.cpp:525-544).
//
// Coarsening, interpolation and the Galerkin product are GLOBAL algorithms here: the
// hierarchy -- and with it the iteration count -- does not depend on the number of ranks.  The first
// implementation got that by replication (every rank built the global hierarchy: O(N_global) memory and time per
// rank, BoomerAMG::build_replicated).  This file builds the SAME hierarchy with O(N_global / P + halo) per rank:
//
//   strength        row-local (row scale and row sum see diag and halo entries alike)
//   PMIS            measures |S^T_i| + rand_i with the halo part of S^T summed back to the owners, rand_i = element i
//                   of the one global Park-Miller stream (jump-ahead by modular exponentiation); every round
//                   exchanges the C/F state of the halo points and sends the "you lose" flags back
//   interpolation   on a per-rank EXTENDED sub-problem: own rows + the rows of the halo points (fetched with
//                   their strength flags) + the second-ring columns those rows touch, numbered in ascending
//                   global order -- so stored order, discovery order and with them every floating-point sum are
//                   the ones of the single-rank algorithm, and the existing routine (hs::build_interp) runs
//                   unchanged on the extended CSR
//   Galerkin        A*P with the P rows of the halo columns fetched from their owners; P^T by an exchange of the
//                   entries whose coarse column lives elsewhere, sent together with the (A*P) row they multiply:
//                   the owner of a coarse row evaluates R*(A*P) itself, in the single-rank order (bit-identical)
//   non-Galerkin    (optional) drop-and-lump on the owner's rows of R A P, with the row maxima of the halo columns
//                   fetched from their owners
//   ordering        C-first renumbering per rank; halo / transfer-operator columns are translated by asking
//                   the owners for the new positions
//
// Levels whose per-rank pieces are large are built on the device (DevLevel below: the same steps on extended index
// spaces, halo-sized pieces through the host); the host loop takes over at the first small level.
//
// Below the redundancy threshold (HYPRE_BoomerAMGSetSeqThreshold) the level is gathered and every rank builds
// the small remaining hierarchy for itself, as before.  Aggressive levels (second-generation PMIS on the C points,
// multipass interpolation pass by pass with the halo rows of the previous pass) are distributed too (host loop).
// HMIS / per-rank Ruge-Stueben / Falgout and CLJP (dist_coarsen) are host passes of this file too; only
// coarsening type 3 (a third Ruge-Stueben pass on the boundary) keeps the replicated path on N > 1.
//
// Shared with the single-rank host setup (amg_setup_internal.hpp), stated once: the strength rule of a row
// (hs::strength_rule), PMIS and CLJP (hs::pmis / hs::cljp over a graph view: DistGraph here, LocalGraph there; only
// CLJP's common-C-point test has a form per view), the Park-Miller stream, and the non-Galerkin drop-and-lump
// (hs::drop_and_lump).  Within this file every halo exchange goes through the two Ring primitives (to_halo /
// to_owners), per-halo-row records through Ring::each_record, and the host loop and the device levels share
// transpose_exchange.  Deliberately still separate pairs: build_multipass / dist_multipass and second_strength /
// dist_second_stage (the distributed forms work pass by pass on fetched halo rows), and hs::build_interp, which runs
// unchanged on the extended sub-problem.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "amg.hpp"
#include "amg_setup_internal.hpp"

namespace mi {
using namespace hs;

namespace {

long long g_ext_rows_max = 0, g_global_rows_gathered = 0, g_dist_setups = 0, g_dev_levels = 0;

// this rank's rows of a distributed operator: GLOBAL column ids, ascending inside a row
struct GlobCSR {
  int nrows = 0;
  std::vector<int64_t> ia;
  std::vector<gidx> gj;
  std::vector<double> a;
  int64_t nnz() const { return ia.empty() ? 0 : ia.back(); }
};

int rank_of_id(const std::vector<gidx> &starts, gidx g) {
  return (int)(std::upper_bound(starts.begin(), starts.end(), g) - starts.begin()) - 1;
}

template <class T>
void put(std::vector<char> &buf, const T *p, size_t n) {
  const size_t off = buf.size();
  buf.resize(off + n * sizeof(T));
  if (n) memcpy(buf.data() + off, p, n * sizeof(T));
}
template <class T>
void put1(std::vector<char> &buf, T v) {
  put(buf, &v, 1);
}
struct Reader {
  const char *p, *e;
  explicit Reader(const std::vector<char> &b) : p(b.data()), e(b.data() + b.size()) {}
  template <class T>
  T get() {
    T v;
    MI_REQUIRE(p + sizeof(T) <= e, "distributed setup: short message");
    memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
  }
  template <class T>
  void get(T *out, size_t n) {
    MI_REQUIRE(p + n * sizeof(T) <= e, "distributed setup: short message");
    if (n) memcpy(out, p, n * sizeof(T));
    p += n * sizeof(T);
  }
  bool done() const { return p >= e; }
};
template <class T>
struct Ragged {  // list q = items[off[q] .. off[q + 1])
  std::vector<int64_t> off{0};
  std::vector<T> items;
};

// Neighbour plan for a sorted set of remote ids of a vector partitioned by `starts`: who owns them (receive side)
// and which of my entries the others asked for (send side).  hypre_ParCSRCommPkg for an arbitrary id set.
struct Ring {
  std::vector<gidx> ids;  // the remote ids, ascending (so the ids of one owner are contiguous)
  std::vector<int> recv_peers, recv_starts, send_peers, send_starts, send_map;
  gidx my0 = 0;

  void build(Comm &comm, const std::vector<gidx> &starts, std::vector<gidx> need) {
    ids.swap(need);
    my0 = starts[(size_t)comm.rank];
    const gidx my1 = starts[(size_t)comm.rank + 1];
    recv_peers.clear(), recv_starts.assign(1, 0), send_peers.clear(), send_starts.assign(1, 0), send_map.clear();
    for (size_t k = 0; k < ids.size(); k++) {
      const int o = rank_of_id(starts, ids[k]);
      MI_REQUIRE(o >= 0 && o < comm.size && o != comm.rank, "distributed setup: remote id without an owner");
      if (recv_peers.empty() || recv_peers.back() != o) {
        if (!recv_peers.empty()) recv_starts.push_back((int)k);
        recv_peers.push_back(o);
      }
    }
    if (!recv_peers.empty()) recv_starts.push_back((int)ids.size());
    if (recv_peers.empty()) recv_starts.assign(1, 0);
    std::vector<std::vector<char>> req(recv_peers.size());
    for (size_t i = 0; i < recv_peers.size(); i++)
      put(req[i], ids.data() + recv_starts[i], (size_t)(recv_starts[i + 1] - recv_starts[i]));
    std::vector<int> from;
    std::vector<std::vector<char>> got;
    comm.exchange_host(recv_peers, req, from, got);
    for (size_t i = 0; i < from.size(); i++) {
      const size_t cnt = got[i].size() / sizeof(gidx);
      const gidx *g = reinterpret_cast<const gidx *>(got[i].data());
      for (size_t k = 0; k < cnt; k++) {
        MI_REQUIRE(g[k] >= my0 && g[k] < my1, "distributed setup: a peer asked for an entry this rank does not own");
        send_map.push_back((int)(g[k] - my0));
      }
      send_peers.push_back(from[i]);
      send_starts.push_back((int)send_map.size());
    }
  }
  int slot_of(gidx g) const {  // position of a remote id in `ids`
    return (int)(std::lower_bound(ids.begin(), ids.end(), g) - ids.begin());
  }
  // The transport under every halo exchange of this file: send[i] goes to to[i], the answers come back indexed by
  // position in `back`.  Every peer of a plan owes at least one entry, so a peer of `back` that stays silent is an error.
  static std::vector<std::vector<char>> transport(Comm &comm, const std::vector<int> &to, const std::vector<std::vector<char>> &send,
                                                  const std::vector<int> &back) {
    std::vector<int> from;
    std::vector<std::vector<char>> got;
    comm.exchange_host(to, send, from, got);
    std::vector<std::vector<char>> out(back.size());
    std::vector<char> heard(back.size(), 0);
    for (size_t i = 0; i < from.size(); i++) {
      const size_t pi = (size_t)(std::find(back.begin(), back.end(), from[i]) - back.begin());
      MI_REQUIRE(pi < back.size(), "distributed setup: unexpected sender");
      out[pi].swap(got[i]);
      heard[pi] = 1;
    }
    MI_REQUIRE(std::find(heard.begin(), heard.end(), 0) == heard.end(), "distributed setup: a halo peer sent nothing");
    return out;
  }
  // the two primitives: byte strings for send_peers -> byte strings by position in recv_peers, and the way back
  std::vector<std::vector<char>> to_halo(Comm &comm, const std::vector<std::vector<char>> &send) const {
    return transport(comm, send_peers, send, recv_peers);
  }
  std::vector<std::vector<char>> to_owners(Comm &comm, const std::vector<std::vector<char>> &send) const {
    return transport(comm, recv_peers, send, send_peers);
  }
  // fixed-size payloads: v is cut at `cuts` into one message per peer / the messages are laid out at `cuts`
  template <class T>
  static std::vector<std::vector<char>> split(const std::vector<T> &v, const std::vector<int> &cuts) {
    std::vector<std::vector<char>> msg(cuts.size() - 1);
    for (size_t i = 0; i + 1 < cuts.size(); i++) put(msg[i], v.data() + cuts[i], (size_t)(cuts[i + 1] - cuts[i]));
    return msg;
  }
  template <class T>
  static std::vector<T> join(const std::vector<std::vector<char>> &msg, const std::vector<int> &cuts) {
    std::vector<T> v((size_t)cuts.back());
    for (size_t i = 0; i < msg.size(); i++) {
      MI_REQUIRE(msg[i].size() == (size_t)(cuts[i + 1] - cuts[i]) * sizeof(T), "distributed setup: halo message of the wrong size");
      memcpy(v.data() + cuts[i], msg[i].data(), msg[i].size());
    }
    return v;
  }
  // values in send_map order -> the halo copies (ids order); one value per halo id -> the owners, in send_map order
  template <class T>
  std::vector<T> forward_packed(Comm &comm, const std::vector<T> &at_send) const {
    return join<T>(to_halo(comm, split(at_send, send_starts)), recv_starts);
  }
  template <class T>
  std::vector<T> reverse_packed(Comm &comm, const std::vector<T> &ext) const {
    return join<T>(to_owners(comm, split(ext, recv_starts)), send_starts);
  }
  // values of my entries -> their halo copies
  template <class T>
  std::vector<T> forward(Comm &comm, const std::vector<T> &local) const {
    std::vector<T> at_send(send_map.size());
    for (size_t k = 0; k < send_map.size(); k++) at_send[k] = local[(size_t)send_map[k]];
    return forward_packed(comm, at_send);
  }
  // one value per halo id -> the owners, folded into their entries
  template <class T, class F>
  void reverse(Comm &comm, const std::vector<T> &ext, std::vector<T> &local, F fold) const {
    const std::vector<T> at_send = reverse_packed(comm, ext);
    for (size_t k = 0; k < send_map.size(); k++) fold(local[(size_t)send_map[k]], at_send[k]);
  }
  // a variable-size record of every row the peers asked for -> per receive peer one byte string holding the
  // records of its ids in ascending id order
  template <class Pack>
  std::vector<std::vector<char>> forward_records(Comm &comm, Pack pack) const {
    std::vector<std::vector<char>> send(send_peers.size());
    for (size_t i = 0; i < send_peers.size(); i++)
      for (int k = send_starts[i]; k < send_starts[i + 1]; k++) pack(send_map[(size_t)k], send[i]);
    return to_halo(comm, send);
  }
  // ... and their reader: read(q, rd) takes the record of halo slot q off the Reader; every string must be used up
  template <class Read>
  void each_record(const std::vector<std::vector<char>> &rec, Read read) const {
    for (size_t pi = 0; pi < rec.size(); pi++) {
      Reader rd(rec[pi]);
      for (int q = recv_starts[pi]; q < recv_starts[pi + 1]; q++) read(q, rd);
      MI_REQUIRE(rd.done(), "distributed setup: halo records longer than their plan");
    }
  }
  // records that are "count, then that many T": the lists of all halo slots, back to back
  template <class T>
  Ragged<T> read_lists(const std::vector<std::vector<char>> &rec) const {
    Ragged<T> r;
    each_record(rec, [&](int, Reader &rd) {
      const size_t len = (size_t)rd.get<int>(), o = r.items.size();
      r.items.resize(o + len);
      rd.get(r.items.data() + o, len);
      r.off.push_back((int64_t)r.items.size());
    });
    return r;
  }
};

// one level of the hierarchy while it is being built (natural ordering, global ids)
struct DLevel {
  std::vector<gidx> starts;  // row partition
  GlobCSR A;
  std::vector<char> strong;  // per entry of A
  Ring ring;                 // halo of A: its remote columns
  std::vector<int> cf;       // local rows (special F already turned into F)
  std::vector<gidx> cgid;    // local rows: global coarse id of a C point, -1 otherwise
  GlobCSR P;                 // my fine rows x global coarse ids
  GlobCSR R;                 // my coarse rows x global fine ids
  bool has_cf = false;
  gidx n0() const { return starts.empty() ? 0 : starts.front(); }
};

// index set {local range} u {sorted remote ids}, numbered in ascending global order
struct ExtIndex {
  gidx s = 0, e = 0;
  std::vector<gidx> remote;  // sorted unique, none in [s, e)
  int nbelow = 0;
  void finish() { nbelow = (int)(std::lower_bound(remote.begin(), remote.end(), s) - remote.begin()); }
  int size() const { return (int)(e - s) + (int)remote.size(); }
  int of(gidx g) const {
    if (g >= s && g < e) return nbelow + (int)(g - s);
    const int q = (int)(std::lower_bound(remote.begin(), remote.end(), g) - remote.begin());
    return g < s ? q : q + (int)(e - s);
  }
  gidx global(int idx) const {
    if (idx < nbelow) return remote[(size_t)idx];
    if (idx < nbelow + (int)(e - s)) return s + (idx - nbelow);
    return remote[(size_t)(idx - (int)(e - s))];
  }
};

void sort_unique(std::vector<gidx> &v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}

// the ids of v outside [lo, hi), appended to out (any order, duplicates kept): almost every id of a block-row
// partition is inside, so the column sets below are "the whole own range + these few"
void append_outside(const std::vector<gidx> &v, gidx lo, gidx hi, std::vector<gidx> &out) {
  std::mutex mu;
  parallel_for((int64_t)v.size(), [&](int64_t b, int64_t en, int) {
    std::vector<gidx> mine;
    for (int64_t k = b; k < en; k++)
      if (v[(size_t)k] < lo || v[(size_t)k] >= hi) mine.push_back(v[(size_t)k]);
    if (!mine.empty()) {
      std::lock_guard<std::mutex> g(mu);
      out.insert(out.end(), mine.begin(), mine.end());
    }
  });
}

// rows in `order` (local row ids; empty = natural), columns translated through `newcol` (one new GLOBAL id per
// entry of M) and sorted, split at this rank's column range into the diag / halo blocks of a ParCSR
std::unique_ptr<ParCSR> assemble_rows(const GlobCSR &M, const std::vector<int> &order, const std::vector<gidx> &newcol,
                                      const std::vector<gidx> &row_starts, const std::vector<gidx> &col_starts, int rank) {
  std::unique_ptr<ParCSR> Q(new ParCSR());
  const int n = M.nrows;
  const gidx c0 = col_starts[(size_t)rank], c1 = col_starts[(size_t)rank + 1];
  Q->nrows = n;
  Q->row_starts = row_starts;
  Q->col_starts = col_starts;
  Q->row_start = row_starts[(size_t)rank];
  Q->row_end = row_starts[(size_t)rank + 1];
  HostCSR &D = Q->diag, &O = Q->offd;
  D.nrows = O.nrows = n;
  D.ncols = (int)(c1 - c0);
  D.ia.assign((size_t)n + 1, 0);
  O.ia.assign((size_t)n + 1, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t q = b; q < e; q++) {
      const int i = order.empty() ? (int)q : order[(size_t)q];
      int nd = 0;
      for (int64_t k = M.ia[(size_t)i]; k < M.ia[(size_t)i + 1]; k++) nd += (newcol[(size_t)k] >= c0 && newcol[(size_t)k] < c1);
      D.ia[(size_t)q + 1] = nd;
      O.ia[(size_t)q + 1] = M.ia[(size_t)i + 1] - M.ia[(size_t)i] - nd;
    }
  });
  for (int q = 0; q < n; q++) {
    D.ia[(size_t)q + 1] += D.ia[(size_t)q];
    O.ia[(size_t)q + 1] += O.ia[(size_t)q];
  }
  D.ja.resize((size_t)D.nnz());
  D.a.resize((size_t)D.nnz());
  O.ja.resize((size_t)O.nnz());
  O.a.resize((size_t)O.nnz());
  std::vector<gidx> ogid((size_t)O.nnz());
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    std::vector<std::pair<gidx, double>> row;
    for (int64_t q = b; q < e; q++) {
      const int i = order.empty() ? (int)q : order[(size_t)q];
      row.clear();
      for (int64_t k = M.ia[(size_t)i]; k < M.ia[(size_t)i + 1]; k++) row.push_back({newcol[(size_t)k], M.a[(size_t)k]});
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
  sort_unique(Q->col_map_offd);
  for (size_t k = 0; k < ogid.size(); k++)
    O.ja[k] = (int)(std::lower_bound(Q->col_map_offd.begin(), Q->col_map_offd.end(), ogid[k]) - Q->col_map_offd.begin());
  O.ncols = (int)Q->col_map_offd.size();
  return Q;
}

// wrap an extended-index CSR as the single-rank operator the host routines expect
void as_single_rank(HostCSR &&M, ParCSR &Q) {
  Q.nrows = M.nrows;
  Q.row_start = 0;
  Q.row_end = M.nrows;
  Q.row_starts = {0, (gidx)M.nrows};
  Q.offd.nrows = M.nrows;
  Q.offd.ncols = 0;
  Q.offd.ia.assign((size_t)M.nrows + 1, 0);
  Q.diag = std::move(M);
}

// C = A * B for the extended sub-problems: the device SpGEMM (same accumulation order, bit-identical:
// tests/test_gpu_setup_kernels.py) when a GPU is in use and the product is large, the threaded host routine otherwise
void spgemm_auto(const HostCSR &A, const HostCSR &B, HostCSR &C, long long device_min_rows) {
  if (device_min_rows >= 0 && A.nrows >= device_min_rows && ctx().inited) {
    hipStream_t s = ctx().stream;
    sk::DCsr dA, dB, dC;
    dA.upload(A, s);
    dB.upload(B, s);
    sk::spgemm(dA, dB, dC, s);
    dA.release();
    dB.release();
    dC.download(C, s);
    C.nrows = A.nrows;
    C.ncols = B.ncols;
    return;
  }
  host_spgemm(A, B, C);
}


// Non-Galerkin sparsification of a distributed operator (hs::sparsify_non_galerkin on this rank's rows): the row maxima
// m_j of the remote columns come from their owners; everything else is row-local, in stored order.
void sparsify_non_galerkin_dist(Comm &comm, GlobCSR &A, const std::vector<gidx> &starts, double tol) {
  const int n = A.nrows;
  const gidx s = starts[(size_t)comm.rank], e = starts[(size_t)comm.rank + 1];
  const std::vector<double> m = offdiag_row_maxima(n, A.ia, A.gj, A.a, s);
  Ring ring;
  {
    std::vector<gidx> need;
    append_outside(A.gj, s, e, need);
    sort_unique(need);
    ring.build(comm, starts, std::move(need));
  }
  const std::vector<double> m_h = ring.forward(comm, m);
  auto m_of = [&](gidx j) { return (j >= s && j < e) ? m[(size_t)(j - s)] : m_h[(size_t)ring.slot_of(j)]; };
  drop_and_lump(n, A.ia, A.gj, A.a, s, m, m_of, tol);
}

// ============================================================================================================
// Device-resident levels (round 3).  The levels of the distributed hierarchy whose per-rank pieces are large are
// built without host copies of the operators: a rank keeps its rows of A, P and R on the device in EXTENDED index
// spaces [remote ids below the own range | own range | remote ids above], ascending in the global id like the
// single-rank numbering.  Every sum is therefore taken in the single-rank order, and the single-rank device
// kernels (sk::strength, sk::interp, sk::spgemm, sk::transpose) run unchanged on the extended matrices; the PMIS
// rounds run on the own rows with the halo state exchanged between the steps (sk::pmis_dist_*).  What crosses the
// host are the halo-sized pieces only: the rows of the halo points, their P rows, the (A P) rows that travel to the
// owners of remote coarse points, and per-point state.  Same hierarchy as build_distributed's host loop bit for bit
// (tests/test_dist.py, device threshold 0).
// ============================================================================================================
struct DevLevel {
  std::vector<gidx> starts;
  ExtIndex E;   // column space of A: own rows + ring-1 halo ids
  sk::DCsr A;   // n x E.size(), natural order
  Ring ring1;   // over E.remote
  ExtIndex CE;  // column space of P: own coarse range + remote coarse ids
  sk::DCsr P;   // n x CE.size()
  ExtIndex E2;  // column space of R: own fine rows + the fine rows of other ranks that reach my coarse points
  sk::DCsr R;   // n_coarse x E2.size()
};

struct RowSet {  // rows with global column ids
  std::vector<int64_t> ia{0};
  std::vector<gidx> col;
  std::vector<double> val;
  int rows() const { return (int)ia.size() - 1; }
};

sk::ExtColMap identity_map(int ncols) {
  sk::ExtColMap m;
  m.nb_old = 0;
  m.n_own = ncols;
  m.own_new0 = 0;
  return m;
}

// position in `to` of every id of `from_remote` (ascending remote ids of another extended space); -1 = not there
void remote_table(const std::vector<gidx> &from_remote, const ExtIndex &to, DVec<int> &tab) {
  std::vector<int> t(from_remote.size());
  const int nown = (int)(to.e - to.s);
  parallel_for((int64_t)from_remote.size(), [&](int64_t b, int64_t e, int) {
    for (int64_t k = b; k < e; k++) {
      const gidx g = from_remote[(size_t)k];
      const size_t q = (size_t)(std::lower_bound(to.remote.begin(), to.remote.end(), g) - to.remote.begin());
      const bool there = q < to.remote.size() && to.remote[q] == g;
      t[(size_t)k] = !there ? -1 : (g < to.s ? (int)q : (int)q + nown);
    }
  });
  tab.upload(t);
}

// own rows keep their place, remote columns move through `tab` (remote_table of from.remote in `to`)
sk::ExtColMap ext_map(const ExtIndex &from, const ExtIndex &to, const DVec<int> &tab) {
  sk::ExtColMap m;
  m.nb_old = from.nbelow;
  m.n_own = (int)(from.e - from.s);
  m.own_new0 = to.nbelow;
  m.below = tab.p;
  m.above = tab.p + from.nbelow;
  return m;
}

// The rows of M (own rows; row r of the partition is row r + row_shift of M; columns in `cols`) that the peers asked
// for through `ring` travel to them as (lengths, global column ids, values); returns the rows of ring.ids (ascending).
RowSet fetch_rows(Comm &comm, const Ring &ring, const sk::DCsr &M, int row_shift, const ExtIndex &cols, hipStream_t s) {
  const int ns = (int)ring.send_map.size();
  HostCSR h;
  h.ia.assign(1, 0);
  if (ns) {
    std::vector<int> rows((size_t)ns);
    for (int k = 0; k < ns; k++) rows[(size_t)k] = ring.send_map[(size_t)k] + row_shift;
    DVec<int> d;
    d.upload(rows);
    sk::DCsr sel;
    sk::select_rows(M, d.p, 0, ns, identity_map(M.ncols), M.ncols, false, sel, s);
    sel.download(h, s);
  }
  std::vector<std::vector<char>> send(ring.send_peers.size());
  for (size_t i = 0; i < ring.send_peers.size(); i++) {
    const int b = ring.send_starts[i], e = ring.send_starts[i + 1];
    std::vector<int> len((size_t)(e - b));
    for (int k = b; k < e; k++) len[(size_t)(k - b)] = (int)(h.ia[(size_t)k + 1] - h.ia[(size_t)k]);
    put(send[i], len.data(), len.size());
    const int64_t e0 = h.ia[(size_t)b], e1 = h.ia[(size_t)e];
    std::vector<gidx> g((size_t)(e1 - e0));
    for (int64_t q = e0; q < e1; q++) g[(size_t)(q - e0)] = cols.global(h.ja[(size_t)q]);
    put(send[i], g.data(), g.size());
    put(send[i], h.a.data() + e0, (size_t)(e1 - e0));
  }
  const std::vector<std::vector<char>> got = ring.to_halo(comm, send);
  RowSet out;
  for (size_t pi = 0; pi < got.size(); pi++) {
    const size_t cnt = (size_t)(ring.recv_starts[pi + 1] - ring.recv_starts[pi]);
    Reader rd(got[pi]);
    std::vector<int> len(cnt);
    rd.get(len.data(), cnt);
    size_t total = 0;
    for (int l : len) total += (size_t)l;
    const size_t off = out.col.size();
    out.col.resize(off + total);
    out.val.resize(off + total);
    rd.get(out.col.data() + off, total);
    rd.get(out.val.data() + off, total);
    for (int l : len) out.ia.push_back(out.ia.back() + l);
  }
  MI_REQUIRE(out.rows() == (int)ring.ids.size(), "distributed setup: halo rows and halo ids disagree");
  return out;
}

// The remote part of an extended ROW space (`space`: ascending remote ids, the first nbelow below the own range) as
// two device blocks: the ids of `have` (an ascending subset) carry the rows of `rs`, the others are empty.
template <class F>
void remote_blocks(const std::vector<gidx> &space, int nbelow, const std::vector<gidx> &have, const RowSet &rs, int ncols,
                   F colmap, sk::DCsr &below, sk::DCsr &above, hipStream_t s) {
  HostCSR B[2];
  B[0].nrows = nbelow;
  B[1].nrows = (int)space.size() - nbelow;
  for (int q = 0; q < 2; q++) {
    B[q].ncols = ncols;
    B[q].ia.assign((size_t)B[q].nrows + 1, 0);
  }
  size_t h = 0;
  for (size_t x = 0; x < space.size(); x++) {
    HostCSR &T = B[(int)x < nbelow ? 0 : 1];
    const size_t r = (int)x < nbelow ? x : x - (size_t)nbelow;
    int64_t len = 0;
    if (h < have.size() && have[h] == space[x]) {
      for (int64_t k = rs.ia[h]; k < rs.ia[h + 1]; k++) {
        T.ja.push_back(colmap(rs.col[(size_t)k]));
        T.a.push_back(rs.val[(size_t)k]);
      }
      len = rs.ia[h + 1] - rs.ia[h];
      h++;
    }
    T.ia[r + 1] = T.ia[r] + len;
  }
  MI_REQUIRE(h == have.size(), "distributed setup: a fetched row has no place in the extended row space");
  below.upload(B[0], s);
  above.upload(B[1], s);
}

// halo exchange of per-point state that lives in a device vector over an extended space (ring.ids = its remote ids)
struct DevHalo {
  Comm &comm;
  const Ring &ring;
  int nb, n, ne;
  hipStream_t s;
  DVec<int> d_send;
  DevHalo(Comm &c, const Ring &r, int nb_, int n_, int ne_, hipStream_t s_) : comm(c), ring(r), nb(nb_), n(n_), ne(ne_), s(s_) {
    MI_REQUIRE((int)ring.ids.size() == ne - n, "distributed setup: halo ring and extended space disagree");
    d_send.upload(ring.send_map);
  }
  // own values -> their copies on the ranks that hold them as remote points
  template <class T>
  void forward(T *vec) {
    const int ns = (int)ring.send_map.size();
    std::vector<T> sv((size_t)ns);
    if (ns) {
      DVec<T> tmp((size_t)ns);
      sk::gather_elems(vec, d_send.p, nb, ns, (int)sizeof(T), tmp.p, s);
      d2h(sv.data(), tmp.p, (size_t)ns * sizeof(T), s);
      MI_HIP(hipStreamSynchronize(s));
    }
    const std::vector<T> ext = ring.forward_packed(comm, sv);
    if (nb) MI_HIP(hipMemcpyAsync(vec, ext.data(), (size_t)nb * sizeof(T), hipMemcpyHostToDevice, s));
    if (ne - n - nb) MI_HIP(hipMemcpyAsync(vec + nb + n, ext.data() + nb, (size_t)(ne - n - nb) * sizeof(T), hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
  }
  // remote values -> the owners; returns, in send_map order, what the peers hold for my points (on the device)
  template <class T>
  void reverse(const T *vec, DVec<T> &at_send) {
    std::vector<T> ext(ring.ids.size());
    if (nb) d2h(ext.data(), vec, (size_t)nb * sizeof(T), s);
    if (ne - n - nb) d2h(ext.data() + nb, vec + nb + n, (size_t)(ne - n - nb) * sizeof(T), s);
    MI_HIP(hipStreamSynchronize(s));
    at_send.upload(ring.reverse_packed(comm, ext));
  }
};

// Transpose exchange of the Galerkin product: the P entries whose coarse column lives on another rank travel to its
// owner together with the (A P) row of their fine row, so that the owner of a coarse row evaluates R (A P) itself.
struct Incoming {
  gidx fine;
  std::vector<gidx> pc;  // coarse ids (the receiver's)
  std::vector<double> pv;
  std::vector<gidx> ac;  // the fine row's (A P) row
  std::vector<double> av;
};
// rows(emit) calls emit(fine global id, P row: global coarse ids (ascending) / values / length, (A P) row: global ids /
// values / length) for the rows of this rank that may reach other ranks, fine ids ascending; next_starts = the coarse
// partition.  Returns what the other ranks sent here, sorted by fine id.
template <class Rows>
std::vector<Incoming> transpose_exchange(Comm &comm, const std::vector<gidx> &next_starts, Rows rows) {
  std::vector<std::vector<char>> out((size_t)comm.size);
  rows([&](gidx fine, const gidx *pc, const double *pv, int64_t np, const gidx *ac, const double *av, int64_t na) {
    for (int64_t k = 0; k < np;) {
      const int o = rank_of_id(next_starts, pc[k]);
      const int64_t k0 = k;
      while (k < np && pc[k] < next_starts[(size_t)o + 1]) k++;  // columns ascend: one owner's run
      if (o == comm.rank) continue;
      std::vector<char> &buf = out[(size_t)o];
      put1<gidx>(buf, fine);
      put1<int>(buf, (int)(k - k0));
      put(buf, pc + k0, (size_t)(k - k0));
      put(buf, pv + k0, (size_t)(k - k0));
      put1<int>(buf, (int)na);
      put(buf, ac, (size_t)na);
      put(buf, av, (size_t)na);
    }
  });
  std::vector<int> peers, from;
  std::vector<std::vector<char>> send, got;
  for (int r = 0; r < comm.size; r++)
    if (!out[(size_t)r].empty()) {
      peers.push_back(r);
      send.emplace_back(std::move(out[(size_t)r]));
    }
  comm.exchange_host(peers, send, from, got);
  std::vector<Incoming> inc;
  for (auto &buf : got) {
    Reader rd(buf);
    while (!rd.done()) {
      inc.emplace_back();
      Incoming &in = inc.back();
      in.fine = rd.get<gidx>();
      const int np = rd.get<int>();
      in.pc.resize((size_t)np), in.pv.resize((size_t)np);
      rd.get(in.pc.data(), (size_t)np);
      rd.get(in.pv.data(), (size_t)np);
      const int na = rd.get<int>();
      in.ac.resize((size_t)na), in.av.resize((size_t)na);
      rd.get(in.ac.data(), (size_t)na);
      rd.get(in.av.data(), (size_t)na);
    }
  }
  std::sort(inc.begin(), inc.end(), [](const Incoming &x, const Incoming &y) { return x.fine < y.fine; });
  return inc;
}

// sorted unique ids of v outside [lo, hi) appended to `out` (kept sorted unique)
void merge_outside(const std::vector<gidx> &v, gidx lo, gidx hi, std::vector<gidx> &out) {
  for (gidx g : v)
    if (g < lo || g >= hi) out.push_back(g);
  sort_unique(out);
}

struct DevBuild {
  std::vector<DevLevel> lev;     // processed levels (each has a splitting, P and R)
  std::vector<std::vector<int>> cf;  // their C/F splittings (special F already F), natural order
  // the first level the device loop did not process: its operator is still on the device
  std::vector<gidx> next_starts;
  ExtIndex next_E;
  sk::DCsr next_A;
};

// level 0 on the device: diag + halo blocks merged into rows of ascending (new) global column ids
void dev_level0(Comm &comm, ParCSR &A0, const std::vector<int> &input_order, const std::vector<int> &newloc,
                const std::vector<gidx> &newcol_h, sk::DCsr &dD, ExtIndex &E, sk::DCsr &A, hipStream_t s) {
  (void)comm;
  const int n = A0.nrows, nh = (int)A0.col_map_offd.size();
  const bool renum = !input_order.empty();
  const std::vector<gidx> &rg = renum ? newcol_h : A0.col_map_offd;
  E.s = A0.row_start, E.e = A0.row_end;
  E.remote = rg;
  sort_unique(E.remote);
  E.finish();
  if (dD.nrows != n) dD.upload(A0.diag, s);
  sk::DCsr dO, cat;
  {
    HostCSR O = A0.offd;  // full-length row pointers
    O.nrows = n;
    O.ncols = nh;
    if (O.ia.empty()) O.ia.assign((size_t)n + 1, 0);
    dO.upload(O, s);
  }
  dD.ncols = n;
  sk::hstack(dD, dO, cat, s);
  dD.release();
  dO.release();
  std::vector<int> colpos((size_t)n + (size_t)nh);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t j = b; j < e; j++) colpos[(size_t)j] = E.nbelow + (renum ? newloc[(size_t)j] : (int)j);
  });
  for (int k = 0; k < nh; k++) colpos[(size_t)n + (size_t)k] = E.of(rg[(size_t)k]);
  DVec<int> dcol, dperm;
  dcol.upload(colpos);
  if (renum) dperm.upload(input_order);
  sk::permute(cat, renum ? dperm.p : nullptr, dcol.p, A, s);
  A.ncols = E.size();
}

// One level on the device.  In: Lv.starts, Lv.E, Lv.A.  Out: the splitting, Lv.P, Lv.R (+ their column spaces), and the
// next level's partition / column space / operator.  Returns false when the coarsening stops here (nothing is built).
bool dev_level(BoomerAMG &amg, Comm &comm, int level, DevLevel &Lv, std::vector<int> &cf_host, std::vector<gidx> &next_starts,
               ExtIndex &next_E, sk::DCsr &next_A, std::map<std::string, double> *sub_times) {
  const AmgParams &p = amg.p;
  hipStream_t s = ctx().stream;
  const int rank = comm.rank, size = comm.size;
  const gidx gs = Lv.starts[(size_t)rank], ge = Lv.starts[(size_t)rank + 1];
  const gidx N = Lv.starts.back();
  const int n = (int)(ge - gs);
  const ExtIndex &E = Lv.E;
  double tsub = wall_time();
  auto lap = [&](const char *what) {
    if (!sub_times) return;
    MI_HIP(hipStreamSynchronize(s));
    const double now = wall_time();
    (*sub_times)[what] += now - tsub;
    tsub = now;
  };
  double tp0 = wall_time();

  // ---- the rows of the halo points, and with them the second ring: extended space X
  Ring ring1;  // over the first ring (the remote columns of my rows)
  ring1.build(comm, Lv.starts, E.remote);
  const std::vector<gidx> ring1_ids = E.remote;
  RowSet hrows = fetch_rows(comm, ring1, Lv.A, 0, E, s);
  lap("device: fetch halo rows");
  ExtIndex X;
  X.s = gs, X.e = ge;
  X.remote = E.remote;
  merge_outside(hrows.col, gs, ge, X.remote);
  X.finish();
  const int ne = X.size(), nbX = X.nbelow;
  g_ext_rows_max = std::max<long long>(g_ext_rows_max, ne);
  sk::DCsr Ae;
  sk::DCsr &AownX = Lv.A;  // from here on the level's rows live in X (in place: the map is monotone and drops nothing)
  {
    DVec<int> tab;
    remote_table(E.remote, X, tab);
    sk::remap_columns(Lv.A, ext_map(E, X, tab), ne, s);
    Lv.E = X;  // (E is Lv.E)
    lap("device: own rows on the extended columns");
    sk::DCsr below, above;
    remote_blocks(X.remote, nbX, ring1_ids, hrows, ne, [&](gidx g) { return X.of(g); }, below, above, s);
    const sk::DCsr *parts[3] = {&below, &AownX, &above};
    sk::vconcat(parts, 3, Ae, s);
  }
  hrows = RowSet();
  lap("device: extended operator");

  // ---- strength (row-local: exact for the own rows and the halo rows, which are whole)
  sk::DCsr Se;
  sk::strength(Ae, p.strong_threshold, p.max_row_sum, Se, s);
  amg.t_phase[0] += wall_time() - tp0;
  lap("device: strength");

  // ---- PMIS on the own rows, halo state exchanged between the steps (see the host loop in build_distributed)
  tp0 = wall_time();
  Ring &ring12 = Lv.ring1;  // over both rings: the halo ring of the level's operator as it is kept (columns in X)
  ring12.build(comm, Lv.starts, X.remote);
  DevHalo halo(comm, ring12, nbX, n, ne, s);
  DVec<int> dcf((size_t)ne), counter(1);
  {
    DVec<int> cnt((size_t)ne);
    DVec<double> measure((size_t)ne);
    DVec<signed char> tmp((size_t)ne);
    MI_HIP(hipMemsetAsync(cnt.p, 0, (size_t)ne * sizeof(int), s));
    MI_HIP(hipMemsetAsync(dcf.p, 0, (size_t)ne * sizeof(int), s));
    MI_HIP(hipMemsetAsync(measure.p, 0, (size_t)ne * sizeof(double), s));
    sk::pmis_dist_counts(Se, nbX, n, cnt.p, s);
    {
      DVec<int> at_send;
      halo.reverse(cnt.p, at_send);
      sk::scatter_add_int(cnt.p, halo.d_send.p, nbX, at_send.p, (int)ring12.send_map.size(), s);
      MI_HIP(hipStreamSynchronize(s));
    }
    long long left = sk::pmis_dist_init(Se, nbX, n, gs, 2747, cnt.p, measure.p, dcf.p, counter.p, s);
    halo.forward(measure.p);
    halo.forward(dcf.p);
    int rounds = 0;
    for (;;) {
      long long glob = left;
      comm.allreduce_host(&glob, 1, CommDType::I64, CommOp::SUM);
      if (glob == 0) break;
      MI_REQUIRE(++rounds <= 10000, "PMIS does not terminate");
      sk::pmis_dist_compare(Se, nbX, n, ne, dcf.p, measure.p, tmp.p, s);
      {
        DVec<signed char> at_send;
        halo.reverse(tmp.p, at_send);
        sk::scatter_zero_flags(tmp.p, halo.d_send.p, nbX, at_send.p, (int)ring12.send_map.size(), s);
        MI_HIP(hipStreamSynchronize(s));
      }
      sk::pmis_dist_select(nbX, n, dcf.p, tmp.p, s);
      halo.forward(dcf.p);
      left = sk::pmis_dist_fpoints(Se, nbX, n, dcf.p, counter.p, s);
      halo.forward(dcf.p);
    }
  }
  DVec<long long> crank;
  const long long nc_loc = sk::count_c_points(dcf.p + nbX, n, crank, s);
  long long nc_glob = nc_loc;
  comm.allreduce_host(&nc_glob, 1, CommDType::I64, CommOp::SUM);
  amg.t_phase[1] += wall_time() - tp0;
  lap("device: pmis");
  if (nc_glob == 0 || nc_glob == N || nc_glob < p.min_coarse_size) return false;

  // ---- coarse partition and the coarse ids of every point of X
  tp0 = wall_time();
  {
    std::vector<long long> all((size_t)size, 0);
    comm.allgather_host(&nc_loc, all.data(), sizeof(long long));
    next_starts.assign((size_t)size + 1, 0);
    for (int r = 0; r < size; r++) next_starts[(size_t)r + 1] = next_starts[(size_t)r] + all[(size_t)r];
  }
  const gidx cs = next_starts[(size_t)rank];
  const int ncl = (int)nc_loc;
  ExtIndex CX;  // the C points of X by coarse id
  CX.s = cs, CX.e = cs + nc_loc;
  {
    DVec<long long> cg((size_t)ne);
    MI_HIP(hipMemsetAsync(cg.p, 0xff, (size_t)ne * sizeof(long long), s));  // -1
    sk::fill_coarse_ids(dcf.p + nbX, crank.p, n, cs, cg.p + nbX, s);
    halo.forward(cg.p);
    std::vector<long long> cgr((size_t)(ne - n));
    if (nbX) d2h(cgr.data(), cg.p, (size_t)nbX * sizeof(long long), s);
    if (ne - n - nbX)
      d2h(cgr.data() + nbX, cg.p + nbX + n, (size_t)(ne - n - nbX) * sizeof(long long), s);
    MI_HIP(hipStreamSynchronize(s));
    for (long long g : cgr)
      if (g >= 0) CX.remote.push_back(g);  // ascending: coarse ids ascend with the fine ids
    CX.finish();
  }
  crank.release();

  // ---- interpolation on the extended sub-problem (every row is computed, the own rows are the ones that count)
  sk::DCsr Pe;
  int nce = 0;
  bool on_dev = (p.interp_type == 6 || p.interp_type == 0) &&
                sk::interp(Ae, Se, dcf, p.interp_type, p.trunc_factor, p.pmax_elmts, Pe, nce, s);
  if (!on_dev) {
    // a row whose interpolatory set outgrows the kernels' tables (or another interpolation type): host routine
    HostCSR Ah, Ph;
    Ae.download(Ah, s);
    Strength Sh;
    Sh.ia.resize((size_t)ne + 1);
    Sh.ja.resize((size_t)Se.nnz);
    d2h(Sh.ia.data(), Se.ia.p, ((size_t)ne + 1) * sizeof(int64_t), s);
    if (Se.nnz) d2h(Sh.ja.data(), Se.ja.p, (size_t)Se.nnz * sizeof(int), s);
    MI_HIP(hipStreamSynchronize(s));
    std::vector<int> cfe = dcf.to_host();
    cfe.resize((size_t)ne);
    std::vector<char> want((size_t)ne, 0);
    for (int i = 0; i < n; i++) want[(size_t)(nbX + i)] = 1;
    ParCSR Aw;
    Ah.nrows = Ah.ncols = ne;
    as_single_rank(std::move(Ah), Aw);
    build_interp(Aw, Sh, cfe, p.interp_type, p.trunc_factor, p.pmax_elmts, Ph, nce, &want);
    for (int &c : cfe)
      if (c == SF_PT) c = F_PT;
    dcf.upload(cfe);
    Ph.nrows = ne;
    Ph.ncols = nce;
    Pe.upload(Ph, s);
  }
  MI_REQUIRE(nce == CX.size(), "distributed setup: coarse point count of the extended sub-problem");
  Se.release();
  Ae.release();
  cf_host.resize((size_t)n);
  if (n) d2h(cf_host.data(), dcf.p + nbX, (size_t)n * sizeof(int), s);
  MI_HIP(hipStreamSynchronize(s));
  for (int &c : cf_host)
    if (c == SF_PT) c = F_PT;
  dcf.release();
  amg.t_phase[2] += wall_time() - tp0;
  lap("device: interpolation");

  // ---- Galerkin product, first half: A P with the P rows of the halo points fetched from their owners
  tp0 = wall_time();
  RowSet prow = fetch_rows(comm, ring1, Pe, nbX, CX, s);
  ExtIndex &CE = Lv.CE;
  CE.s = cs, CE.e = cs + nc_loc;
  CE.remote = CX.remote;
  merge_outside(prow.col, CE.s, CE.e, CE.remote);
  CE.finish();
  sk::DCsr AP;
  {
    DVec<int> tab;
    remote_table(CX.remote, CE, tab);
    sk::select_rows(Pe, nullptr, nbX, n, ext_map(CX, CE, tab), CE.size(), false, Lv.P, s);
    Pe.release();
    sk::DCsr below, above, P1;
    remote_blocks(X.remote, nbX, ring1_ids, prow, CE.size(), [&](gidx g) { return CE.of(g); }, below, above, s);
    const sk::DCsr *parts[3] = {&below, &Lv.P, &above};
    sk::vconcat(parts, 3, P1, s);
    sk::spgemm(AownX, P1, AP, s);
  }
  lap("device: A*P");

  // ---- transpose exchange: P entries whose coarse column lives elsewhere travel to its owner with the (A P) row
  std::vector<Incoming> inc;
  {
    std::vector<int> brows;
    const int nbr = sk::rows_with_columns_outside(Lv.P, CE.nbelow, CE.nbelow + ncl, brows, s);
    HostCSR hp, ha;
    hp.ia.assign(1, 0), ha.ia.assign(1, 0);
    if (nbr) {
      DVec<int> d;
      d.upload(brows);
      sk::DCsr sp, sa;
      sk::select_rows(Lv.P, d.p, 0, nbr, identity_map(Lv.P.ncols), Lv.P.ncols, false, sp, s);
      sk::select_rows(AP, d.p, 0, nbr, identity_map(AP.ncols), AP.ncols, false, sa, s);
      sp.download(hp, s);
      sa.download(ha, s);
    }
    std::vector<gidx> pg(hp.ja.size()), ag(ha.ja.size());  // the downloaded blocks' columns as global coarse ids
    for (size_t k = 0; k < pg.size(); k++) pg[k] = CE.global(hp.ja[k]);
    for (size_t k = 0; k < ag.size(); k++) ag[k] = CE.global(ha.ja[k]);
    inc = transpose_exchange(comm, next_starts, [&](auto emit) {
      for (int q = 0; q < nbr; q++) {
        const int64_t pb = hp.ia[(size_t)q], ab = ha.ia[(size_t)q];
        emit(gs + brows[(size_t)q], pg.data() + pb, hp.a.data() + pb, hp.ia[(size_t)q + 1] - pb, ag.data() + ab, ha.a.data() + ab,
             ha.ia[(size_t)q + 1] - ab);
      }
    });
  }
  lap("device: transpose exchange");

  // ---- second half: R (A P) on my coarse rows
  ExtIndex &E2 = Lv.E2;
  E2.s = gs, E2.e = ge;
  E2.remote.clear();
  for (auto &in : inc) E2.remote.push_back(in.fine);
  E2.finish();
  const int n2 = E2.size();
  g_ext_rows_max = std::max<long long>(g_ext_rows_max, n2);
  ExtIndex CE2;
  CE2.s = cs, CE2.e = cs + nc_loc;
  CE2.remote = CE.remote;
  for (auto &in : inc)
    for (gidx g : in.ac)
      if (g < CE2.s || g >= CE2.e) CE2.remote.push_back(g);
  sort_unique(CE2.remote);
  CE2.finish();
  RowSet inc_ap, inc_p;
  for (auto &in : inc) {
    inc_ap.col.insert(inc_ap.col.end(), in.ac.begin(), in.ac.end());
    inc_ap.val.insert(inc_ap.val.end(), in.av.begin(), in.av.end());
    inc_ap.ia.push_back((int64_t)inc_ap.col.size());
    inc_p.col.insert(inc_p.col.end(), in.pc.begin(), in.pc.end());
    inc_p.val.insert(inc_p.val.end(), in.pv.begin(), in.pv.end());
    inc_p.ia.push_back((int64_t)inc_p.col.size());
  }
  std::vector<Incoming>().swap(inc);
  sk::DCsr Ac;
  {
    sk::DCsr APe2, P2;
    {
      DVec<int> tab;
      remote_table(CE.remote, CE2, tab);
      sk::DCsr below, above;
      sk::remap_columns(AP, ext_map(CE, CE2, tab), CE2.size(), s);
      remote_blocks(E2.remote, E2.nbelow, E2.remote, inc_ap, CE2.size(), [&](gidx g) { return CE2.of(g); }, below, above, s);
      const sk::DCsr *parts[3] = {&below, &AP, &above};
      if (E2.remote.empty()) {
        APe2 = std::move(AP);  // nobody sent rows: the product itself
      } else {
        sk::vconcat(parts, 3, APe2, s);
        AP.release();
      }
    }
    {
      sk::ExtColMap m;  // own coarse columns only, as local coarse ids
      m.nb_old = CE.nbelow;
      m.n_own = ncl;
      m.own_new0 = 0;
      sk::DCsr own, below, above;
      sk::select_rows(Lv.P, nullptr, 0, n, m, ncl, false, own, s);
      remote_blocks(E2.remote, E2.nbelow, E2.remote, inc_p, ncl, [&](gidx g) { return (int)(g - cs); }, below, above, s);
      const sk::DCsr *parts[3] = {&below, &own, &above};
      sk::vconcat(parts, 3, P2, s);
    }
    sk::transpose(P2, Lv.R, s);  // my coarse rows x extended fine rows, ascending
    P2.release();
    sk::spgemm(Lv.R, APe2, Ac, s);
  }
  lap("device: R*(A*P)");
  if (p.non_galerkin_tol_for(level) > 0.0) {
    // non-Galerkin coarse operator: the row maxima of the remote columns come from their owners
    Ring rc;
    rc.build(comm, next_starts, CE2.remote);
    DevHalo hc(comm, rc, CE2.nbelow, ncl, CE2.size(), s);
    DVec<double> m((size_t)CE2.size());
    MI_HIP(hipMemsetAsync(m.p, 0, (size_t)CE2.size() * sizeof(double), s));
    sk::non_galerkin_row_maxima(Ac, CE2.nbelow, m.p, s);
    hc.forward(m.p);
    sk::sparsify_non_galerkin(Ac, p.non_galerkin_tol_for(level), s, CE2.nbelow, m.p);
    lap("device: non-Galerkin sparsification");
  }

  // ---- the next level's column space: the remote coarse ids that occur
  next_E.s = cs, next_E.e = cs + nc_loc;
  next_E.remote.clear();
  {
    DVec<unsigned char> used;
    sk::mark_used_columns(Ac, used, s);
    const int nrem = (int)CE2.remote.size();
    std::vector<unsigned char> u((size_t)nrem);
    if (CE2.nbelow) d2h(u.data(), used.p, (size_t)CE2.nbelow, s);
    if (nrem - CE2.nbelow)
      d2h(u.data() + CE2.nbelow, used.p + CE2.nbelow + ncl, (size_t)(nrem - CE2.nbelow), s);
    MI_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < nrem; k++)
      if (u[(size_t)k]) next_E.remote.push_back(CE2.remote[(size_t)k]);
    next_E.finish();
    DVec<int> tab;
    remote_table(CE2.remote, next_E, tab);
    sk::remap_columns(Ac, ext_map(CE2, next_E, tab), next_E.size(), s);  // (the unused columns have no image: they do not occur)
    next_A = std::move(Ac);
  }
  amg.t_phase[3] += wall_time() - tp0;
  lap("device: next operator");
  return true;
}

// A device level's operator M (rows: own rows of `row level`, columns: extended space `cols` of the `column level`) in
// the final per-rank form: rows in `row_perm` order (empty = natural), own columns through `col_pos` (empty =
// identity), remote columns to the new global ids `newg` (one per id of cols.remote), split into the diag block (on
// the device, `diag_out`) and the halo block (host).  amg_setup_dist.cpp assemble_rows for operators that never were
// on the host.
std::unique_ptr<ParCSR> assemble_dev(const sk::DCsr &M, const ExtIndex &cols, const std::vector<int> &row_perm,
                                     const std::vector<int> &col_pos, const std::vector<gidx> &newg,
                                     const std::vector<gidx> &row_starts, const std::vector<gidx> &col_starts, int rank,
                                     sk::DCsr &diag_out, hipStream_t s) {
  std::unique_ptr<ParCSR> Q(new ParCSR());
  const int n = M.nrows;
  const int ncown = (int)(cols.e - cols.s);
  Q->nrows = n;
  Q->row_starts = row_starts;
  Q->col_starts = col_starts;
  Q->row_start = row_starts[(size_t)rank];
  Q->row_end = row_starts[(size_t)rank + 1];
  // halo columns = the remote ids that occur (the column space may hold more: second-ring points, coarse points
  // nobody interpolates from)
  std::vector<unsigned char> used(newg.size(), 0);
  {
    DVec<unsigned char> du;
    sk::mark_used_columns(M, du, s);
    const size_t nrem = newg.size(), nbl = (size_t)cols.nbelow;
    if (nbl) d2h(used.data(), du.p, nbl, s);
    if (nrem - nbl) d2h(used.data() + nbl, du.p + nbl + (size_t)ncown, nrem - nbl, s);
    MI_HIP(hipStreamSynchronize(s));
  }
  for (size_t k = 0; k < newg.size(); k++)
    if (used[k]) Q->col_map_offd.push_back(newg[k]);
  sort_unique(Q->col_map_offd);
  std::vector<int> tab(newg.size());
  for (size_t k = 0; k < newg.size(); k++)
    tab[k] = !used[k] ? -1
                      : (int)(std::lower_bound(Q->col_map_offd.begin(), Q->col_map_offd.end(), newg[k]) - Q->col_map_offd.begin());
  DVec<int> dtab, dperm, dpos;
  dtab.upload(tab);
  if (!row_perm.empty()) dperm.upload(row_perm);
  if (!col_pos.empty()) dpos.upload(col_pos);
  sk::ExtColMap md;
  md.nb_old = cols.nbelow;
  md.n_own = ncown;
  md.own_new0 = 0;
  md.own_tab = col_pos.empty() ? nullptr : dpos.p;
  sk::select_rows(M, row_perm.empty() ? nullptr : dperm.p, 0, n, md, ncown, !col_pos.empty(), diag_out, s);
  sk::ExtColMap mo;
  mo.nb_old = cols.nbelow;
  mo.n_own = ncown;
  mo.keep_own = false;
  mo.below = dtab.p;
  mo.above = dtab.p + cols.nbelow;
  sk::DCsr off;
  sk::select_rows(M, row_perm.empty() ? nullptr : dperm.p, 0, n, mo, (int)Q->col_map_offd.size(), true, off, s);
  off.download(Q->offd, s);
  Q->offd.nrows = n;
  Q->offd.ncols = (int)Q->col_map_offd.size();
  Q->diag.nrows = n;
  Q->diag.ncols = ncown;
  Q->host_diag_stale = true;
  Q->dev_diag_nnz = diag_out.nnz;
  return Q;
}


// The graph view of the coarsening core (hs::pmis / hs::cljp, amg_setup_internal.hpp) for a distributed graph: this
// rank's rows [starts[rank], starts[rank+1]) with GLOBAL column ids, `strong` = per-entry flag (null: every entry
// counts), `ring` = the plan over the remote columns, `hslot` = halo slot per entry (-1: own column).  Used on the
// strength graph of a level and on the second-generation graph of an aggressive level.
struct DistGraph {
  static constexpr bool has_halo = true;
  Comm &comm;
  const gidx s;
  const int nrows;
  const std::vector<int64_t> &ia;
  const std::vector<gidx> &gj;
  const char *strong;
  const Ring &ring;
  const std::vector<int> &hslot;
  Ragged<gidx> hrow;  // strong rows of the halo points, global column ids (CLJP)
  int n() const { return nrows; }
  int nh() const { return (int)ring.ids.size(); }
  int64_t nnz() const { return ia.empty() ? 0 : ia[(size_t)nrows]; }
  gidx first_id() const { return s; }
  template <class F>
  bool each(int i, F f) const {
    for (int64_t k = ia[(size_t)i]; k < ia[(size_t)i + 1]; k++) {
      if (strong && !strong[(size_t)k]) continue;
      const int h = hslot[(size_t)k];
      if (f(k, h < 0 ? (int)(gj[(size_t)k] - s) : -1, h)) return true;
    }
    return false;
  }
  template <class T>
  void forward(const std::vector<T> &local, std::vector<T> &ext) const {
    ext = ring.forward(comm, local);
  }
  template <class T, class F>
  void reverse(const std::vector<T> &ext, std::vector<T> &local, F fold) const {
    ring.reverse(comm, ext, local, fold);
  }
  long long global_sum(long long v) const {
    comm.allreduce_host(&v, 1, CommDType::I64, CommOp::SUM);
    return v;
  }
  // CLJP H2, "do rows i and j share a C point": sorted-list form.  The C points of row i are collected as global ids
  // (ascending, like the row) and looked up by binary search in the strong row of j -- an own row, or the row of a
  // halo point fetched once.  (LocalGraph in amg_setup.cpp keeps the marker-array form: on one rank every C point has
  // a local index to mark, which is cheaper; here it may lie two rings away and has none.)
  using Marks = std::vector<gidx>;
  void fetch_strong_halo_rows() {
    hrow = ring.read_lists<gidx>(ring.forward_records(comm, [&](int row, std::vector<char> &buf) {
      int cnt = 0;
      for (int64_t k = ia[(size_t)row]; k < ia[(size_t)row + 1]; k++) cnt += (!strong || strong[(size_t)k]);
      put1<int>(buf, cnt);
      for (int64_t k = ia[(size_t)row]; k < ia[(size_t)row + 1]; k++)
        if (!strong || strong[(size_t)k]) put1<gidx>(buf, gj[(size_t)k]);
    }));
  }
  std::vector<Marks> make_marks() const { return std::vector<Marks>((size_t)host_threads()); }
  void begin_row(Marks &mk, int) const { mk.clear(); }
  void mark(Marks &mk, int, int64_t k, int) const { mk.push_back(gj[(size_t)k]); }
  bool shares(const Marks &mk, int, int j, int h) const {
    if (h < 0) {
      for (int64_t kk = ia[(size_t)j]; kk < ia[(size_t)j + 1]; kk++)
        if ((!strong || strong[(size_t)kk]) && std::binary_search(mk.begin(), mk.end(), gj[(size_t)kk])) return true;
      return false;
    }
    for (int64_t t = hrow.off[(size_t)h]; t < hrow.off[(size_t)h + 1]; t++)
      if (std::binary_search(mk.begin(), mk.end(), hrow.items[(size_t)t])) return true;
    return false;
  }
};

// Coarsening of a distributed graph by type.  8 / 9: PMIS.  The types HYPRE defines PER PROCESSOR (par_coarsen.c
// hypre_BoomerAMGCoarsenRuge / ...HMIS; oracle/oracle.c coarsen_by_type_parts): 11 = first Ruge-Stueben pass and 1 = both
// passes on this rank's own graph (strong connections between own points; no boundary treatment), 10 = HMIS = the
// first pass per rank, then PMIS from that state on the global graph.  (6 / 3 -- Falgout, a third pass on the
// boundary -- and CLJP keep their global, sequential form: replicated setup.)
void dist_coarsen(Comm &comm, int type, const std::vector<gidx> &starts, int n, const std::vector<int64_t> &ia,
                  const std::vector<gidx> &gj, const char *strong, const Ring &ring, const std::vector<int> &hslot,
                  std::vector<int> &cf, std::vector<int> &cf_h) {
  const gidx s = starts[(size_t)comm.rank];
  DistGraph g{comm, s, n, ia, gj, strong, ring, hslot, {}};
  if (type == 8 || type == 9) {
    pmis(g, cf, cf_h);
    return;
  }
  if (type == 0 || type == 7) {  // CLJP: a global algorithm whose rounds commute -- the same splitting on any partition
    cljp(g, cf, cf_h);
    return;
  }
  MI_REQUIRE(type == 10 || type == 11 || type == 1 || type == 6, "distributed setup: coarsening type without a distributed form");
  Strength Sl;
  Sl.ia.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) {
    int64_t c = 0;
    for (int64_t k = ia[(size_t)i]; k < ia[(size_t)i + 1]; k++) c += ((!strong || strong[(size_t)k]) && hslot[(size_t)k] < 0);
    Sl.ia[(size_t)i + 1] = Sl.ia[(size_t)i] + c;
  }
  Sl.ja.resize((size_t)Sl.ia[(size_t)n]);
  parallel_for(n, [&](int64_t b, int64_t en, int) {
    for (int64_t i = b; i < en; i++) {
      int64_t w = Sl.ia[(size_t)i];
      for (int64_t k = ia[(size_t)i]; k < ia[(size_t)i + 1]; k++)
        if ((!strong || strong[(size_t)k]) && hslot[(size_t)k] < 0) Sl.ja[(size_t)w++] = (int)(gj[(size_t)k] - s);
    }
  });
  std::vector<int> cf0;
  if (n > 0) ruge_stueben(n, Sl, type == 1 || type == 6, cf0);
  if (type == 10) {
    pmis(g, cf, cf_h, &cf0);
  } else if (type == 6) {  // Falgout: CLJP on the boundary from the interior verdicts
    cljp(g, cf, cf_h, &cf0);
  } else {
    cf.swap(cf0);
    cf_h = ring.forward(comm, cf);
  }
}

// Second stage of aggressive coarsening on N ranks (par_strength.c hypre_BoomerAMGCreate2ndS with num_paths 1, then
// hypre_BoomerAMGCorrectCFMarker; oracle/oracle.c second_strength / coarsen_aggressive; src/HypreSystem.cpp:215-219).
// The C points of the first PMIS get global ids in fine order (owner of the point = owner of the id); C point i
// depends on C point j != i iff j is in S_i or in S_k for some k in S_i.  The S rows of the halo points arrive as
// lists of first-stage coarse ids; the graph's rows are sorted global ids, its remote columns (C points up to two
// rings away) get a plan of their own, and the same distributed PMIS runs on it with the random stream indexed by
// the coarse id.  A first-stage C point the second stage rejects takes the second stage's verdict.
void dist_second_stage(Comm &comm, int type, const std::vector<gidx> &starts, const GlobCSR &A, const std::vector<char> &strong,
                       const Ring &ring, const std::vector<int> &hslot, std::vector<int> &cf, std::vector<int> &cf_h) {
  const int rank = comm.rank, size = comm.size;
  const int n = A.nrows;
  const gidx s = starts[(size_t)rank];
  long long nc1 = 0;
  for (int i = 0; i < n; i++) nc1 += (cf[(size_t)i] == C_PT);
  std::vector<gidx> st1((size_t)size + 1, 0);
  {
    std::vector<long long> all((size_t)size, 0);
    comm.allgather_host(&nc1, all.data(), sizeof(long long));
    for (int r = 0; r < size; r++) st1[(size_t)r + 1] = st1[(size_t)r] + all[(size_t)r];
  }
  const gidx c0 = st1[(size_t)rank];
  std::vector<gidx> cg1((size_t)n, -1);
  std::vector<int> crow((size_t)nc1);
  {
    int q = 0;
    for (int i = 0; i < n; i++)
      if (cf[(size_t)i] == C_PT) {
        crow[(size_t)q] = i;
        cg1[(size_t)i] = c0 + q++;
      }
  }
  const std::vector<gidx> cg1_h = ring.forward(comm, cg1);
  auto cg_of = [&](int64_t k) {
    const int h = hslot[(size_t)k];
    return h < 0 ? cg1[(size_t)(A.gj[(size_t)k] - s)] : cg1_h[(size_t)h];
  };
  // the strong C neighbours of every halo point, as first-stage coarse ids
  const Ragged<gidx> hl = ring.read_lists<gidx>(ring.forward_records(comm, [&](int row, std::vector<char> &buf) {
    int cnt = 0;
    for (int64_t k = A.ia[(size_t)row]; k < A.ia[(size_t)row + 1]; k++) cnt += (strong[(size_t)k] && cg_of(k) >= 0);
    put1<int>(buf, cnt);
    for (int64_t k = A.ia[(size_t)row]; k < A.ia[(size_t)row + 1]; k++)
      if (strong[(size_t)k] && cg_of(k) >= 0) put1<gidx>(buf, cg_of(k));
  }));
  // rows of the second-generation graph: sorted global coarse ids, the point itself left out
  GlobCSR G;
  G.nrows = (int)nc1;
  G.ia.assign((size_t)nc1 + 1, 0);
  std::vector<std::vector<gidx>> rows((size_t)nc1);
  parallel_for(nc1, [&](int64_t b, int64_t en, int) {
    for (int64_t ci = b; ci < en; ci++) {
      const int i = crow[(size_t)ci];
      const gidx me = c0 + ci;
      std::vector<gidx> &row = rows[(size_t)ci];
      for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) {
        if (!strong[(size_t)k]) continue;
        const gidx g1 = cg_of(k);
        if (g1 >= 0 && g1 != me) row.push_back(g1);
        const int h = hslot[(size_t)k];
        if (h < 0) {
          const int j = (int)(A.gj[(size_t)k] - s);
          for (int64_t kk = A.ia[(size_t)j]; kk < A.ia[(size_t)j + 1]; kk++) {
            if (!strong[(size_t)kk]) continue;
            const gidx g2 = cg_of(kk);
            if (g2 >= 0 && g2 != me) row.push_back(g2);
          }
        } else {
          for (int64_t t = hl.off[(size_t)h]; t < hl.off[(size_t)h + 1]; t++)
            if (hl.items[(size_t)t] != me) row.push_back(hl.items[(size_t)t]);
        }
      }
      std::sort(row.begin(), row.end());
      row.erase(std::unique(row.begin(), row.end()), row.end());
      G.ia[(size_t)ci + 1] = (int64_t)row.size();
    }
  });
  for (long long q = 0; q < nc1; q++) G.ia[(size_t)q + 1] += G.ia[(size_t)q];
  G.gj.resize((size_t)G.nnz());
  parallel_for(nc1, [&](int64_t b, int64_t en, int) {
    for (int64_t ci = b; ci < en; ci++)
      if (!rows[(size_t)ci].empty())
        memcpy(G.gj.data() + G.ia[(size_t)ci], rows[(size_t)ci].data(), rows[(size_t)ci].size() * sizeof(gidx));
  });
  std::vector<std::vector<gidx>>().swap(rows);
  Ring ring2;
  {
    std::vector<gidx> need;
    append_outside(G.gj, c0, c0 + nc1, need);
    sort_unique(need);
    ring2.build(comm, st1, std::move(need));
  }
  std::vector<int> hslot2((size_t)G.nnz(), -1);
  parallel_for((int64_t)G.gj.size(), [&](int64_t b, int64_t en, int) {
    for (int64_t k = b; k < en; k++)
      if (G.gj[(size_t)k] < c0 || G.gj[(size_t)k] >= c0 + nc1) hslot2[(size_t)k] = ring2.slot_of(G.gj[(size_t)k]);
  });
  g_ext_rows_max = std::max<long long>(g_ext_rows_max, nc1 + (long long)ring2.ids.size());
  std::vector<int> cf2, cf2_h;
  dist_coarsen(comm, type, st1, (int)nc1, G.ia, G.gj, nullptr, ring2, hslot2, cf2, cf2_h);
  for (long long q = 0; q < nc1; q++)
    if (cf2[(size_t)q] != C_PT) cf[(size_t)crow[(size_t)q]] = cf2[(size_t)q];
  cf_h = ring.forward(comm, cf);
}

// Multipass interpolation on N ranks (par_multi_interp.c hypre_BoomerAMGBuildMultipass; formulas and order of
// operations: oracle/oracle.c build_multipass; the interpolation of aggressive levels, agg_interp_type 4,
// src/HypreSystem.cpp:220-224, and interp_type 4).  Pass k builds the rows of the F points with a strong neighbour
// reached in pass k-1 THROUGH those neighbours' rows; for halo neighbours the rows (global coarse ids and weights in
// discovery order, untruncated -- what the single-rank routine reads) and the pass numbers arrive after every pass.
// Every row is accumulated by one thread in the column order of A's row (ascending global ids = the single-rank
// order), so the weights are the single-rank ones bit for bit.  Truncation and the sort by coarse id follow the last pass.
void dist_multipass(Comm &comm, const std::vector<gidx> &starts, const GlobCSR &A, const std::vector<char> &strong,
                    const Ring &ring, const std::vector<int> &hslot, const std::vector<int> &cf, const std::vector<int> &cf_h,
                    const std::vector<gidx> &cgid, const std::vector<gidx> &cgid_h, double trunc_factor, int pmax, GlobCSR &P) {
  const int n = A.nrows;
  const gidx s = starts[(size_t)comm.rank];
  const int nh = (int)ring.ids.size();
  std::vector<int> assigned((size_t)n, -1), assigned_h((size_t)nh, -1), rlen((size_t)n, 0), hlen((size_t)nh, 0);
  std::vector<int64_t> rstart((size_t)n, 0), hstart((size_t)nh, 0);
  std::vector<gidx> pool_c, hpool_c;  // own rows in the order they were built / halo rows of the previous pass
  std::vector<double> pool_v, hpool_v;
  pool_c.reserve((size_t)n);
  pool_v.reserve((size_t)n);
  for (int i = 0; i < n; i++)
    if (cf[(size_t)i] == C_PT) {
      assigned[(size_t)i] = 0;
      rstart[(size_t)i] = (int64_t)pool_c.size();
      rlen[(size_t)i] = 1;
      pool_c.push_back(cgid[(size_t)i]);
      pool_v.push_back(1.0);
    }
  for (int q = 0; q < nh; q++)
    if (cf_h[(size_t)q] == C_PT) {
      assigned_h[(size_t)q] = 0;
      hstart[(size_t)q] = (int64_t)hpool_c.size();
      hlen[(size_t)q] = 1;
      hpool_c.push_back(cgid_h[(size_t)q]);
      hpool_v.push_back(1.0);
    }
  std::vector<int> list;
  for (int pass = 1;; pass++) {
    list.clear();
    for (int i = 0; i < n; i++) {
      if (assigned[(size_t)i] != -1 || cf[(size_t)i] == SF_PT) continue;
      for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) {
        if (!strong[(size_t)k]) continue;
        const int h = hslot[(size_t)k];
        if ((h < 0 ? assigned[(size_t)(A.gj[(size_t)k] - s)] : assigned_h[(size_t)h]) == pass - 1) {
          list.push_back(i);
          break;
        }
      }
    }
    const int64_t nl = (int64_t)list.size();
    long long nl_glob = nl;
    comm.allreduce_host(&nl_glob, 1, CommDType::I64, CommOp::SUM);
    if (nl_glob == 0) break;  // the rest cannot be reached along strong connections
    RowCollector<gidx> rows(nl);
    parallel_for(nl, [&](int64_t b, int64_t e, int t) {
      auto &out = rows.begin(t, b);
      std::vector<gidx> &oc = out.j;
      std::vector<double> &ov = out.a;
      std::vector<std::pair<gidx, int>> seen;  // coarse id -> position in the row (rows are short: sorted insert)
      for (int64_t q = b; q < e; q++) {
        const int i = list[(size_t)q];
        const size_t base = oc.size();
        seen.clear();
        double diagonal = 0.0, sum_N = 0.0, sum_J = 0.0;
        for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) {
          if (A.gj[(size_t)k] == s + i) {
            diagonal = A.a[(size_t)k];
            continue;
          }
          sum_N += A.a[(size_t)k];
          if (!strong[(size_t)k]) continue;
          const int h = hslot[(size_t)k];
          const gidx *rc;
          const double *rv;
          int len;
          if (h < 0) {
            const int j = (int)(A.gj[(size_t)k] - s);
            if (assigned[(size_t)j] != pass - 1) continue;
            rc = pool_c.data() + rstart[(size_t)j], rv = pool_v.data() + rstart[(size_t)j], len = rlen[(size_t)j];
          } else {
            if (assigned_h[(size_t)h] != pass - 1) continue;
            rc = hpool_c.data() + hstart[(size_t)h], rv = hpool_v.data() + hstart[(size_t)h], len = hlen[(size_t)h];
          }
          sum_J += A.a[(size_t)k];
          for (int w = 0; w < len; w++) {
            const gidx c = rc[w];
            auto it = std::lower_bound(seen.begin(), seen.end(), std::make_pair(c, -1));
            int pos;
            if (it == seen.end() || it->first != c) {
              pos = (int)(oc.size() - base);
              seen.insert(it, std::make_pair(c, pos));
              oc.push_back(c);
              ov.push_back(0.0);
            } else
              pos = it->second;
            ov[base + (size_t)pos] += A.a[(size_t)k] * rv[w];
          }
        }
        const double alfa = (sum_J * diagonal != 0.0) ? -sum_N / (sum_J * diagonal) : 0.0;
        const int len = (int)(oc.size() - base);
        for (int w = 0; w < len; w++) ov[base + (size_t)w] *= alfa;
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
    // the halo points reached in this pass, with their rows
    assigned_h = ring.forward(comm, assigned);
    const std::vector<std::vector<char>> rec = ring.forward_records(comm, [&](int row, std::vector<char> &buf) {
      const int len = assigned[(size_t)row] == pass ? rlen[(size_t)row] : 0;
      put1<int>(buf, len);
      put(buf, pool_c.data() + rstart[(size_t)row], (size_t)len);
      put(buf, pool_v.data() + rstart[(size_t)row], (size_t)len);
    });
    hpool_c.clear(), hpool_v.clear();
    ring.each_record(rec, [&](int q, Reader &rd) {
      const int len = rd.get<int>();
      const size_t o = hpool_c.size();
      hstart[(size_t)q] = (int64_t)o;
      hlen[(size_t)q] = len;
      hpool_c.resize(o + (size_t)len);
      hpool_v.resize(o + (size_t)len);
      rd.get(hpool_c.data() + o, (size_t)len);
      rd.get(hpool_v.data() + o, (size_t)len);
    });
  }
  // truncation and sort row by row (in place in the pool), then compaction into P
  std::vector<int> flen((size_t)n, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    std::vector<char> keep;
    std::vector<int> idx;
    std::vector<gidx> tmpc;
    for (int64_t i = b; i < e; i++) {
      int len = rlen[(size_t)i];
      gidx *rc = pool_c.data() + rstart[(size_t)i];
      double *rv = pool_v.data() + rstart[(size_t)i];
      if (cf[(size_t)i] != C_PT && len > 0) {
        idx.resize((size_t)len);
        for (int w = 0; w < len; w++) idx[(size_t)w] = w;
        tmpc.assign(rc, rc + len);
        len = truncate_row(len, idx.data(), rv, trunc_factor, pmax, keep);
        for (int w = 0; w < len; w++) rc[w] = tmpc[(size_t)idx[(size_t)w]];
      }
      for (int a = 1; a < len; a++) {
        const gidx c = rc[a];
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
  P.ia.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) P.ia[(size_t)i + 1] = P.ia[(size_t)i] + flen[(size_t)i];
  P.gj.resize((size_t)P.nnz());
  P.a.resize((size_t)P.nnz());
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      if (!flen[(size_t)i]) continue;
      memcpy(P.gj.data() + P.ia[(size_t)i], pool_c.data() + rstart[(size_t)i], (size_t)flen[(size_t)i] * sizeof(gidx));
      memcpy(P.a.data() + P.ia[(size_t)i], pool_v.data() + rstart[(size_t)i], (size_t)flen[(size_t)i] * sizeof(double));
    }
  });
}

}  // namespace

long long dist_setup_counter(const char *name) {
  const std::string n(name);
  if (n == "setup_ext_rows_max") return g_ext_rows_max;
  if (n == "setup_global_rows_gathered") return g_global_rows_gathered;
  if (n == "setup_distributed") return g_dist_setups;
  if (n == "setup_device_levels") return g_dev_levels;  // levels of the distributed setup that were built on the device
  return -1;
}
void dist_setup_counters_reset() { g_ext_rows_max = g_global_rows_gathered = g_dist_setups = g_dev_levels = 0; }

bool BoomerAMG::can_build_distributed() const {
  static const bool forced_off = getenv("MI_HYPRE_REPLICATED_SETUP") && atoi(getenv("MI_HYPRE_REPLICATED_SETUP")) != 0;
  // PMIS splittings, every interpolation this library has (multipass and the second-generation PMIS of aggressive
  // levels pass by pass with halo rows since round 3), Galerkin or non-Galerkin coarse operators.  The Ruge-Stueben
  // family and CLJP are sequential sweeps over the GLOBAL graph in this library's specification: replicated.
  // Coarsening types 10 / 11 / 1 / 6 are PER-RANK algorithms by HYPRE's definition (dist_coarsen): only the distributed
  // setup builds them on N > 1, whatever the switch says.  CLJP (0 / 7) is global and distributed like PMIS; type 3
  // (a third Ruge-Stueben pass on the boundary) is the one left to the replicated setup.
  // The two-stage extended interpolation of aggressive levels (agg_interp_type 5) has no distributed form yet: such
  // hierarchies are built replicated, whatever the coarsening type.
  if (p.agg_num_levels > 0 && p.agg_interp_type == 5) return false;
  // nor has the matrix-matrix extended interpolation (interp_type 16 / 17)
  if (p.interp_type == 16 || p.interp_type == 17) return false;
  // nor has one-point interpolation (interp_type 100)
  if (p.interp_type == 100) return false;
  if (p.coarsen_type == 10 || p.coarsen_type == 11 || p.coarsen_type == 1 || p.coarsen_type == 6) return true;
  return !forced_off && (p.coarsen_type == 8 || p.coarsen_type == 9 || p.coarsen_type == 0 || p.coarsen_type == 7);
}

void BoomerAMG::build_distributed(ParCSR &A0) {
  Comm &comm = my_comm();
  const int rank = comm.rank, size = comm.size;
  g_dist_setups++;
  std::vector<DLevel> D;
  D.reserve((size_t)std::max(2, p.max_levels + 1));
  D.emplace_back();
  D[0].starts = A0.row_starts;
  // internal locality numbering of this rank's rows (BoomerAMG::use_locality_order): clusters of the diag-block
  // graph, rows with halo entries last; the halo columns follow their owners' renumbering (one exchange)
  input_order.clear();
  std::vector<int> order_h;  // (host vector while the hierarchy is built; BoomerAMG::input_order at the end)
  const double t_begin = wall_time();
  std::vector<int> newloc;       // old local row -> new local row
  std::vector<gidx> newcol_h;    // new GLOBAL id of every halo column of A0
  // Large per-rank pieces are built on the device (DevLevel above): decided per level by the SMALLEST piece, so that
  // every rank takes the same path; MI_HYPRE_DIST_DEVICE_SETUP=0 keeps every level on the host loop below
  static const bool dev_enabled = !(getenv("MI_HYPRE_DIST_DEVICE_SETUP") && atoi(getenv("MI_HYPRE_DIST_DEVICE_SETUP")) == 0);
  auto smallest_piece = [&](long long n) {
    long long m = n;
    comm.allreduce_host(&m, 1, CommDType::I64, CommOp::MIN);
    return m;
  };
  // (aggressive levels come first and are host passes -- second-generation PMIS, multipass interpolation -- and the
  // device loop cannot resume after a host level: hierarchies with aggressive levels stay on the host loop)
  const bool dev_candidate = dev_enabled && device_min_rows >= 0 && ctx().inited && (p.interp_type == 6 || p.interp_type == 0) &&
                             p.agg_num_levels <= 0 && (p.coarsen_type == 8 || p.coarsen_type == 9);  // (PMIS is what the device loop runs)
  const bool dev_path = dev_candidate && smallest_piece(A0.nrows) >= std::max<long long>(1, device_min_rows);
  sk::DCsr dD0;  // the diag block of A0 in the setup format, when the device path starts from the copy in HBM
  if (dev_path && A0.on_device && A0.d_diag.nrows == A0.nrows && A0.d_diag.nnz == A0.diag.nnz() && !A0.d_diag.rowmap.p)
    sk::from_solve_format(A0.d_diag, dD0, ctx().stream);
  if (use_locality_order(A0)) {
    const int n = A0.nrows;
    std::vector<char> has_halo((size_t)n, 0);
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      for (int64_t i = b; i < e; i++) has_halo[(size_t)i] = A0.offd.ia[(size_t)i + 1] > A0.offd.ia[(size_t)i];
    });
    if (dev_path) {
      // the clustering rounds on the device (same labels: tests/test_locality_order.py), rows with halo entries excluded
      hipStream_t s = ctx().stream;
      if (dD0.nrows != n) dD0.upload(A0.diag, s);
      const int segshift = locality_segment_shift(A0.diag);
      const std::vector<int> seeds = locality_seeds(n, segshift, &has_halo);
      std::vector<int> label;
      sk::locality_labels(dD0, seeds.data(), (int)seeds.size(), reinterpret_cast<const unsigned char *>(has_halo.data()), segshift,
                          LOCALITY_MAX_ROUNDS, label, s);
      locality_sort(label, (int)seeds.size(), order_h);
    } else {
      locality_order(A0.diag, order_h, &has_halo);
    }
    newloc.resize((size_t)n);
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      for (int64_t q = b; q < e; q++) newloc[(size_t)order_h[(size_t)q]] = (int)q;
    });
    Ring r0;
    r0.build(comm, A0.row_starts, A0.col_map_offd);
    const std::vector<int> ext = r0.forward(comm, newloc);
    newcol_h.resize(A0.col_map_offd.size());
    for (size_t k = 0; k < newcol_h.size(); k++)
      newcol_h[k] = A0.row_starts[(size_t)rank_of_id(A0.row_starts, A0.col_map_offd[k])] + ext[k];
  }
  const bool sub_timing = getenv("MI_HYPRE_SETUP_TIMING") != nullptr && rank == 0;
  std::map<std::string, double> sub_times;
  const long long red_rows = effective_redundant_rows();
  bool has_tail = false;
  int l = 0;
  DevBuild DB;
  if (dev_path) {
    // ---- the large levels, on the device
    hipStream_t s = ctx().stream;
    const double tl0 = wall_time();
    if (sub_timing) sub_times["prologue: locality numbering, new halo ids"] += tl0 - t_begin;
    DevLevel cur;
    cur.starts = A0.row_starts;
    dev_level0(comm, A0, order_h, newloc, newcol_h, dD0, cur.E, cur.A, s);
    if (sub_timing) sub_times["device: level 0 from the assembled blocks"] += wall_time() - tl0;
    while (l < p.max_levels - 1 && cur.starts.back() > p.max_coarse_size) {
      if (red_rows > 0 && l >= 1 && cur.starts.back() <= red_rows) break;  // the host loop below sets has_tail
      if (l > 0 && smallest_piece(cur.A.nrows) < std::max<long long>(1, device_min_rows)) break;
      std::vector<int> cf;
      DevLevel nxt;
      if (!dev_level(*this, comm, l, cur, cf, nxt.starts, nxt.E, nxt.A, sub_timing ? &sub_times : nullptr)) break;
      DB.lev.push_back(std::move(cur));
      DB.cf.push_back(std::move(cf));
      cur = std::move(nxt);
      l++;
    }
    // the first level the device loop left alone goes to the host loop in global ids
    D.resize((size_t)l + 1);
    for (int q = 0; q < l; q++) {
      D[(size_t)q].starts = DB.lev[(size_t)q].starts;
      D[(size_t)q].cf = std::move(DB.cf[(size_t)q]);
      D[(size_t)q].has_cf = true;
    }
    DLevel &H = D[(size_t)l];
    H.starts = cur.starts;
    const double th0 = wall_time();
    HostCSR h;
    cur.A.download(h, s);
    cur.A.release();
    H.A.nrows = h.nrows;
    H.A.ia.swap(h.ia);
    H.A.a.swap(h.a);
    H.A.gj.resize(h.ja.size());
    const ExtIndex &Ec = cur.E;
    parallel_for((int64_t)h.ja.size(), [&](int64_t b, int64_t e, int) {
      for (int64_t k = b; k < e; k++) H.A.gj[(size_t)k] = Ec.global(h.ja[(size_t)k]);
    });
    if (H.A.ia.empty()) H.A.ia.assign(1, 0);
    if (sub_timing) sub_times["device: hand-over of the first host level"] += wall_time() - th0;
  }
  dD0.release();
  const int n_dev_levels = l;
  g_dev_levels += n_dev_levels;
  if (!dev_path) {  // level 0: diag + halo blocks merged into one row of ascending global columns
    GlobCSR &G = D[0].A;
    const int n = A0.nrows;
    G.nrows = n;
    G.ia.assign((size_t)n + 1, 0);
    const bool renum = !order_h.empty();
    for (int q = 0; q < n; q++) {
      const int i = renum ? order_h[(size_t)q] : q;
      G.ia[(size_t)q + 1] = G.ia[(size_t)q] + (A0.diag.ia[(size_t)i + 1] - A0.diag.ia[(size_t)i]) +
                            (A0.offd.ia[(size_t)i + 1] - A0.offd.ia[(size_t)i]);
    }
    G.gj.resize((size_t)G.nnz());
    G.a.resize((size_t)G.nnz());
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      std::vector<std::pair<gidx, double>> row;
      for (int64_t q = b; q < e; q++) {
        const int i = renum ? order_h[(size_t)q] : (int)q;
        row.clear();
        for (int64_t k = A0.diag.ia[(size_t)i]; k < A0.diag.ia[(size_t)i + 1]; k++)
          row.push_back({A0.row_start + (renum ? newloc[(size_t)A0.diag.ja[(size_t)k]] : A0.diag.ja[(size_t)k]), A0.diag.a[(size_t)k]});
        for (int64_t k = A0.offd.ia[(size_t)i]; k < A0.offd.ia[(size_t)i + 1]; k++)
          row.push_back({renum ? newcol_h[(size_t)A0.offd.ja[(size_t)k]] : A0.col_map_offd[(size_t)A0.offd.ja[(size_t)k]],
                         A0.offd.a[(size_t)k]});
        std::sort(row.begin(), row.end(),
                  [](const std::pair<gidx, double> &x, const std::pair<gidx, double> &y) { return x.first < y.first; });
        int64_t w = G.ia[(size_t)q];
        for (auto &en : row) {
          G.gj[(size_t)w] = en.first;
          G.a[(size_t)w++] = en.second;
        }
      }
    });
  }
  double tp0;
  double tsub = 0.0;
  auto lap = [&](const char *what) {
    if (!sub_timing) return;
    const double now = wall_time();
    sub_times[what] += now - tsub;
    tsub = now;
  };
  while (l < p.max_levels - 1 && D[(size_t)l].starts.back() > p.max_coarse_size) {
    if (red_rows > 0 && l >= 1 && D[(size_t)l].starts.back() <= red_rows) {
      has_tail = true;
      break;
    }
    DLevel &Lv = D[(size_t)l];
    const GlobCSR &A = Lv.A;
    const int n = A.nrows;
    const gidx s = Lv.starts[(size_t)rank], e = Lv.starts[(size_t)rank + 1];
    const gidx N = Lv.starts.back();
    MI_REQUIRE((gidx)n == e - s, "distributed setup: partition and rows disagree");

    // ---- strength (par_strength.c), row-local
    tp0 = wall_time();
    Lv.strong.assign((size_t)A.nnz(), 0);
    parallel_for(n, [&](int64_t b, int64_t en, int) {
      for (int64_t i = b; i < en; i++) {
        const int64_t r0 = A.ia[(size_t)i], r1 = A.ia[(size_t)i + 1];
        int64_t dpos = -1;
        for (int64_t k = r0; k < r1; k++)
          if (A.gj[(size_t)k] == s + i) dpos = k;
        const StrengthRule rule = strength_rule(A.a.data() + r0, r1 - r0, dpos < 0 ? -1 : dpos - r0, p.strong_threshold, p.max_row_sum);
        for (int64_t k = r0; k < r1; k++) Lv.strong[(size_t)k] = (k != dpos && rule(A.a[(size_t)k]));
      }
    });
    // halo of A
    {
      std::vector<gidx> need;
      append_outside(A.gj, s, e, need);
      sort_unique(need);
      Lv.ring.build(comm, Lv.starts, std::move(need));
    }
    const Ring &ring = Lv.ring;
    const int nh = (int)ring.ids.size();
    // halo slot of every remote entry of A (reused by every pass below)
    std::vector<int> hslot((size_t)A.nnz(), -1);
    parallel_for(n, [&](int64_t b, int64_t en, int) {
      for (int64_t i = b; i < en; i++)
        for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++)
          if (A.gj[(size_t)k] < s || A.gj[(size_t)k] >= e) hslot[(size_t)k] = ring.slot_of(A.gj[(size_t)k]);
    });
    t_phase[0] += wall_time() - tp0;

    // ---- PMIS on the global graph (par_coarsen.c), one global random stream
    tp0 = wall_time();
    tsub = tp0;
    std::vector<int> cf, cf_h;
    dist_coarsen(comm, p.coarsen_type, Lv.starts, n, A.ia, A.gj, Lv.strong.data(), ring, hslot, cf, cf_h);
    lap("pmis: rounds");
    // aggressive level (level < agg_num_levels, src/HypreSystem.cpp:215-219): the C points are coarsened once more on
    // the second-generation graph; interpolation is multipass there (and wherever interp_type 4 asks for it)
    const bool aggressive = l < p.agg_num_levels;
    const bool multipass = aggressive || p.interp_type == 4;
    if (aggressive) {
      dist_second_stage(comm, p.coarsen_type, Lv.starts, A, Lv.strong, ring, hslot, cf, cf_h);
      lap("pmis: second generation");
    }
    long long nc_loc = 0;
    for (int i = 0; i < n; i++) nc_loc += (cf[(size_t)i] == C_PT);
    long long nc_glob = nc_loc;
    comm.allreduce_host(&nc_glob, 1, CommDType::I64, CommOp::SUM);
    t_phase[1] += wall_time() - tp0;
    if (nc_glob == 0 || nc_glob == N || nc_glob < p.min_coarse_size) break;

    // ---- coarse partition: the owner of a C point owns its coarse unknown
    tp0 = wall_time();
    D.emplace_back();  // D was reserved: Lv / A / ring stay valid
    DLevel &Ln = D[(size_t)l + 1];
    {
      std::vector<long long> all((size_t)size, 0);
      comm.allgather_host(&nc_loc, all.data(), sizeof(long long));
      Ln.starts.assign((size_t)size + 1, 0);
      for (int r = 0; r < size; r++) Ln.starts[(size_t)r + 1] = Ln.starts[(size_t)r] + all[(size_t)r];
    }
    const gidx cs = Ln.starts[(size_t)rank];
    Lv.cgid.assign((size_t)n, -1);
    {
      gidx q = cs;
      for (int i = 0; i < n; i++)
        if (cf[(size_t)i] == C_PT) Lv.cgid[(size_t)i] = q++;
    }
    const std::vector<gidx> cgid_h = ring.forward(comm, Lv.cgid);

    tsub = wall_time();
    if (multipass) {
      // ---- multipass interpolation, pass by pass with the halo rows of the previous pass
      dist_multipass(comm, Lv.starts, A, Lv.strong, ring, hslot, cf, cf_h, Lv.cgid, cgid_h,
                     aggressive ? p.agg_trunc_factor : p.trunc_factor, aggressive ? p.agg_pmax_elmts : p.pmax_elmts, Lv.P);
      lap("interp: multipass");
    } else {
    // ---- interpolation on the extended sub-problem
    // rows of the halo points with, per entry, strength flag, C/F state and coarse id of the column
    std::vector<std::vector<char>> hrows = ring.forward_records(comm, [&](int row, std::vector<char> &buf) {
      const int64_t b = A.ia[(size_t)row], len = A.ia[(size_t)row + 1] - b;
      put1<int>(buf, (int)len);
      put(buf, A.gj.data() + b, (size_t)len);
      put(buf, A.a.data() + b, (size_t)len);
      put(buf, Lv.strong.data() + b, (size_t)len);
      for (int64_t k = b; k < b + len; k++) {
        const int h = hslot[(size_t)k];
        put1<int>(buf, h < 0 ? cf[(size_t)(A.gj[(size_t)k] - s)] : cf_h[(size_t)h]);
        put1<gidx>(buf, h < 0 ? Lv.cgid[(size_t)(A.gj[(size_t)k] - s)] : cgid_h[(size_t)h]);
      }
    });
    lap("interp: fetch halo rows");
    struct HRow {
      std::vector<gidx> col, cg;
      std::vector<double> val;
      std::vector<char> strong;
      std::vector<int> cfc;
    };
    std::vector<HRow> H((size_t)nh);
    {
      ExtIndex X;
      X.s = s, X.e = e;
      X.remote = ring.ids;
      ring.each_record(hrows, [&](int q, Reader &rd) {
        HRow &hr = H[(size_t)q];
        const int len = rd.get<int>();
        hr.col.resize((size_t)len), hr.val.resize((size_t)len), hr.strong.resize((size_t)len);
        hr.cfc.resize((size_t)len), hr.cg.resize((size_t)len);
        rd.get(hr.col.data(), (size_t)len);
        rd.get(hr.val.data(), (size_t)len);
        rd.get(hr.strong.data(), (size_t)len);
        for (int k = 0; k < len; k++) {
          hr.cfc[(size_t)k] = rd.get<int>();
          hr.cg[(size_t)k] = rd.get<gidx>();
          if (hr.col[(size_t)k] < s || hr.col[(size_t)k] >= e) X.remote.push_back(hr.col[(size_t)k]);
        }
      });
      std::vector<std::vector<char>>().swap(hrows);
      lap("interp: unpack halo rows");
      sort_unique(X.remote);
      X.finish();
      const int ne = X.size();
      g_ext_rows_max = std::max<long long>(g_ext_rows_max, ne);
      // extended operator, strength pattern, C/F state and coarse ids
      HostCSR Ae;
      Strength Se;
      Ae.nrows = Ae.ncols = ne;
      Ae.ia.assign((size_t)ne + 1, 0);
      Se.ia.assign((size_t)ne + 1, 0);
      std::vector<int> cfe((size_t)ne, F_PT);
      std::vector<gidx> cge((size_t)ne, -1);
      std::vector<char> want((size_t)ne, 0);
      std::vector<int> hext((size_t)nh);
      for (int q = 0; q < nh; q++) hext[(size_t)q] = X.of(ring.ids[(size_t)q]);
      parallel_for(n, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++) {
          const int x = X.nbelow + (int)i;
          Ae.ia[(size_t)x + 1] = A.ia[(size_t)i + 1] - A.ia[(size_t)i];
          int ns = 0;
          for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++) ns += Lv.strong[(size_t)k];
          Se.ia[(size_t)x + 1] = ns;
          cfe[(size_t)x] = cf[(size_t)i];
          cge[(size_t)x] = Lv.cgid[(size_t)i];
          want[(size_t)x] = 1;
        }
      });
      std::vector<char> known(want);  // own rows and first-ring halo points: state known from the exchanges above
      for (int q = 0; q < nh; q++) {
        const int x = hext[(size_t)q];
        known[(size_t)x] = 1;
        Ae.ia[(size_t)x + 1] = (int64_t)H[(size_t)q].col.size();
        int ns = 0;
        for (char f : H[(size_t)q].strong) ns += f;
        Se.ia[(size_t)x + 1] = ns;
        cfe[(size_t)x] = cf_h[(size_t)q];
        cge[(size_t)x] = cgid_h[(size_t)q];
      }
      for (int x = 0; x < ne; x++) {
        Ae.ia[(size_t)x + 1] += Ae.ia[(size_t)x];
        Se.ia[(size_t)x + 1] += Se.ia[(size_t)x];
      }
      Ae.ja.resize((size_t)Ae.nnz());
      Ae.a.resize((size_t)Ae.nnz());
      Se.ja.resize((size_t)Se.ia[(size_t)ne]);
      parallel_for(n, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++) {
          const int x = X.nbelow + (int)i;
          int64_t w = Ae.ia[(size_t)x], ws = Se.ia[(size_t)x];
          for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++, w++) {
            const int h = hslot[(size_t)k];
            const int c = h < 0 ? X.nbelow + (int)(A.gj[(size_t)k] - s) : hext[(size_t)h];
            Ae.ja[(size_t)w] = c;
            Ae.a[(size_t)w] = A.a[(size_t)k];
            if (Lv.strong[(size_t)k]) Se.ja[(size_t)ws++] = c;
          }
        }
      });
      for (int q = 0; q < nh; q++) {
        const HRow &hr = H[(size_t)q];
        const int x = hext[(size_t)q];
        int64_t w = Ae.ia[(size_t)x], ws = Se.ia[(size_t)x];
        for (size_t k = 0; k < hr.col.size(); k++, w++) {
          const int c = X.of(hr.col[k]);
          Ae.ja[(size_t)w] = c;
          Ae.a[(size_t)w] = hr.val[k];
          if (hr.strong[k]) Se.ja[(size_t)ws++] = c;
          if (!known[(size_t)c]) {  // a second-ring column: its state came with the row
            cfe[(size_t)c] = hr.cfc[k];
            cge[(size_t)c] = hr.cg[k];
          }
        }
      }
      std::vector<HRow>().swap(H);
      lap("interp: extended sub-problem");
      HostCSR Pe;
      int nce = 0;
      bool p_on_device = false;
      if (device_min_rows >= 0 && ne >= device_min_rows && ctx().inited && (p.interp_type == 6 || p.interp_type == 0)) {
        // the device routine of the single-rank setup (bit-identical rows, tests/test_gpu_setup_kernels.py) on the
        // extended sub-problem; it computes every row, the rows that are not wanted (halo rows, whose own
        // neighbourhood is incomplete here) are simply not read below
        hipStream_t st = ctx().stream;
        sk::DCsr dA, dS, dP;
        dA.upload(Ae, st);
        dS.nrows = dS.ncols = ne;
        dS.nnz = (int64_t)Se.ja.size();
        dS.ia.alloc((size_t)ne + 1);
        dS.ja.alloc(Se.ja.size());
        MI_HIP(hipMemcpyAsync(dS.ia.p, Se.ia.data(), ((size_t)ne + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
        if (!Se.ja.empty())
          MI_HIP(hipMemcpyAsync(dS.ja.p, Se.ja.data(), Se.ja.size() * sizeof(int), hipMemcpyHostToDevice, st));
        DVec<int> dcf;
        dcf.upload(cfe);
        p_on_device = sk::interp(dA, dS, dcf, p.interp_type, p.trunc_factor, p.pmax_elmts, dP, nce, st);
        if (p_on_device) dP.download(Pe, st);
      }
      if (!p_on_device) {
        ParCSR Aw;
        as_single_rank(std::move(Ae), Aw);
        build_interp(Aw, Se, cfe, p.interp_type, p.trunc_factor, p.pmax_elmts, Pe, nce, &want);
      }
      lap("interp: build_interp");
      // extended coarse index -> global coarse id (both ascend with the fine id)
      std::vector<gidx> cmap((size_t)nce);
      {
        int q = 0;
        for (int x = 0; x < ne; x++)
          if (cfe[(size_t)x] == C_PT) cmap[(size_t)q++] = cge[(size_t)x];
        MI_REQUIRE(q == nce, "distributed setup: coarse point count of the extended sub-problem");
      }
      GlobCSR &P = Lv.P;
      P.nrows = n;
      P.ia.assign((size_t)n + 1, 0);
      for (int i = 0; i < n; i++)
        P.ia[(size_t)i + 1] = P.ia[(size_t)i] + (Pe.ia[(size_t)(X.nbelow + i) + 1] - Pe.ia[(size_t)(X.nbelow + i)]);
      P.gj.resize((size_t)P.nnz());
      P.a.resize((size_t)P.nnz());
      std::atomic<int> bad{0};
      parallel_for(n, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++) {
          int64_t w = P.ia[(size_t)i];
          for (int64_t k = Pe.ia[(size_t)(X.nbelow + i)]; k < Pe.ia[(size_t)(X.nbelow + i) + 1]; k++, w++) {
            P.gj[(size_t)w] = cmap[(size_t)Pe.ja[(size_t)k]];
            if (P.gj[(size_t)w] < 0) bad = 1;
            P.a[(size_t)w] = Pe.a[(size_t)k];
          }
        }
      });
      MI_REQUIRE(bad == 0, "distributed setup: interpolation from a point without a coarse id");
    }
    }  // (extended sub-problem)
    for (int i = 0; i < n; i++)
      if (cf[(size_t)i] == SF_PT) cf[(size_t)i] = F_PT;
    Lv.cf = cf;
    Lv.has_cf = true;
    lap("interp: P to global ids");
    t_phase[2] += wall_time() - tp0;

    // ---- Galerkin product A_c = R (A P), every row in the single-rank order
    tp0 = wall_time();
    tsub = tp0;
    const GlobCSR &P = Lv.P;
    GlobCSR AP;  // my fine rows x global coarse ids
    {
      std::vector<std::vector<char>> prow = ring.forward_records(comm, [&](int row, std::vector<char> &buf) {
        const int64_t b = P.ia[(size_t)row], len = P.ia[(size_t)row + 1] - b;
        put1<int>(buf, (int)len);
        put(buf, P.gj.data() + b, (size_t)len);
        put(buf, P.a.data() + b, (size_t)len);
      });
      lap("galerkin: fetch P rows");
      // P restricted to rows {own} u {halo of A}, in ascending global row order
      ExtIndex E1;
      E1.s = s, E1.e = e, E1.remote = ring.ids;
      E1.finish();
      const int n1 = E1.size();
      HostCSR Pe;
      Pe.nrows = n1;
      Pe.ia.assign((size_t)n1 + 1, 0);
      std::vector<std::vector<gidx>> hc((size_t)nh);
      std::vector<std::vector<double>> hv((size_t)nh);
      ring.each_record(prow, [&](int q, Reader &rd) {
        const int len = rd.get<int>();
        hc[(size_t)q].resize((size_t)len), hv[(size_t)q].resize((size_t)len);
        rd.get(hc[(size_t)q].data(), (size_t)len);
        rd.get(hv[(size_t)q].data(), (size_t)len);
      });
      lap("galerkin: unpack P rows");
      // coarse columns of the extended P: my whole coarse range plus the remote ids that occur (ascending global
      // order, as in the single-rank product)
      ExtIndex CE;
      CE.s = cs, CE.e = cs + nc_loc;
      append_outside(P.gj, CE.s, CE.e, CE.remote);
      for (auto &v : hc) append_outside(v, CE.s, CE.e, CE.remote);
      sort_unique(CE.remote);
      CE.finish();
      auto cidx = [&](gidx g) { return CE.of(g); };
      lap("galerkin: coarse column set of P");
      for (int x = 0; x < n1; x++) {
        const gidx g = E1.global(x);
        const int64_t len = (g >= s && g < e) ? P.ia[(size_t)(g - s) + 1] - P.ia[(size_t)(g - s)]
                                               : (int64_t)hc[(size_t)ring.slot_of(g)].size();
        Pe.ia[(size_t)x + 1] = Pe.ia[(size_t)x] + len;
      }
      Pe.ncols = CE.size();
      Pe.ja.resize((size_t)Pe.nnz());
      Pe.a.resize((size_t)Pe.nnz());
      parallel_for(n1, [&](int64_t b, int64_t en, int) {
        for (int64_t x = b; x < en; x++) {
          const gidx g = E1.global((int)x);
          int64_t w = Pe.ia[(size_t)x];
          if (g >= s && g < e) {
            for (int64_t k = P.ia[(size_t)(g - s)]; k < P.ia[(size_t)(g - s) + 1]; k++, w++) {
              Pe.ja[(size_t)w] = cidx(P.gj[(size_t)k]);
              Pe.a[(size_t)w] = P.a[(size_t)k];
            }
          } else {
            const int q = ring.slot_of(g);
            for (size_t k = 0; k < hc[(size_t)q].size(); k++, w++) {
              Pe.ja[(size_t)w] = cidx(hc[(size_t)q][k]);
              Pe.a[(size_t)w] = hv[(size_t)q][k];
            }
          }
        }
      });
      lap("galerkin: extended P");
      HostCSR Ae;
      Ae.nrows = n;
      Ae.ncols = n1;
      Ae.ia.assign(A.ia.begin(), A.ia.end());
      Ae.a = A.a;
      Ae.ja.resize((size_t)A.nnz());
      std::vector<int> hext((size_t)nh);
      for (int q = 0; q < nh; q++) hext[(size_t)q] = E1.of(ring.ids[(size_t)q]);
      parallel_for(n, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++)
          for (int64_t k = A.ia[(size_t)i]; k < A.ia[(size_t)i + 1]; k++)
            Ae.ja[(size_t)k] = hslot[(size_t)k] < 0 ? E1.nbelow + (int)(A.gj[(size_t)k] - s) : hext[(size_t)hslot[(size_t)k]];
      });
      lap("galerkin: A on extended columns");
      HostCSR APe;
      spgemm_auto(Ae, Pe, APe, device_min_rows);
      lap("galerkin: A*P");
      AP.nrows = n;
      AP.ia = APe.ia;
      AP.a.swap(APe.a);
      AP.gj.resize(APe.ja.size());
      parallel_for((int64_t)APe.ja.size(), [&](int64_t b, int64_t en, int) {
        for (int64_t k = b; k < en; k++) AP.gj[(size_t)k] = CE.global(APe.ja[(size_t)k]);
      });
    }
    lap("galerkin: A*P to global ids");
    // transpose exchange: P entries whose coarse column lives elsewhere travel to its owner together with the
    // (A P) row of their fine row
    const std::vector<Incoming> inc = transpose_exchange(comm, Ln.starts, [&](auto emit) {
      for (int i = 0; i < n; i++) {
        const int64_t pb = P.ia[(size_t)i], ab = AP.ia[(size_t)i];
        emit(s + i, P.gj.data() + pb, P.a.data() + pb, P.ia[(size_t)i + 1] - pb, AP.gj.data() + ab, AP.a.data() + ab,
             AP.ia[(size_t)i + 1] - ab);
      }
    });
    lap("galerkin: transpose exchange");
    {
      const int ncl = (int)nc_loc;
      ExtIndex E2;  // fine rows that reach my coarse rows: own rows + the senders' rows
      E2.s = s, E2.e = e;
      for (auto &in : inc) E2.remote.push_back(in.fine);
      E2.finish();
      const int n2 = E2.size();
      g_ext_rows_max = std::max<long long>(g_ext_rows_max, n2);
      ExtIndex CE2;  // coarse columns of the extended A*P: my coarse range plus the remote ids that occur
      CE2.s = cs, CE2.e = cs + nc_loc;
      append_outside(AP.gj, CE2.s, CE2.e, CE2.remote);
      for (auto &in : inc) append_outside(in.ac, CE2.s, CE2.e, CE2.remote);
      sort_unique(CE2.remote);
      CE2.finish();
      auto cidx = [&](gidx g) { return CE2.of(g); };
      lap("galerkin: coarse column set of A*P");
      // (A P) on the extended fine rows
      HostCSR APe;
      APe.nrows = n2;
      APe.ncols = CE2.size();
      APe.ia.assign((size_t)n2 + 1, 0);
      auto inc_of = [&](int x) -> const Incoming & { return inc[(size_t)(x < E2.nbelow ? x : x - n)]; };
      for (int x = 0; x < n2; x++) {
        const bool own = x >= E2.nbelow && x < E2.nbelow + n;
        const int64_t len = own ? AP.ia[(size_t)(x - E2.nbelow) + 1] - AP.ia[(size_t)(x - E2.nbelow)] : (int64_t)inc_of(x).ac.size();
        APe.ia[(size_t)x + 1] = APe.ia[(size_t)x] + len;
      }
      APe.ja.resize((size_t)APe.nnz());
      APe.a.resize((size_t)APe.nnz());
      parallel_for(n2, [&](int64_t b, int64_t en, int) {
        for (int64_t x = b; x < en; x++) {
          int64_t w = APe.ia[(size_t)x];
          if (x >= E2.nbelow && x < E2.nbelow + n) {
            const int64_t i = x - E2.nbelow;
            for (int64_t k = AP.ia[(size_t)i]; k < AP.ia[(size_t)i + 1]; k++, w++) {
              APe.ja[(size_t)w] = cidx(AP.gj[(size_t)k]);
              APe.a[(size_t)w] = AP.a[(size_t)k];
            }
          } else {
            const Incoming &in = inc_of((int)x);
            for (size_t k = 0; k < in.ac.size(); k++, w++) {
              APe.ja[(size_t)w] = cidx(in.ac[k]);
              APe.a[(size_t)w] = in.av[k];
            }
          }
        }
      });
      lap("galerkin: extended A*P");
      // R = P^T restricted to my coarse rows, columns = extended fine rows (ascending)
      HostCSR Re;
      Re.nrows = ncl;
      Re.ncols = n2;
      Re.ia.assign((size_t)ncl + 1, 0);
      auto each_entry = [&](auto &&f) {  // (coarse local row, extended fine index, value), fine index ascending
        for (int x = 0; x < n2; x++) {
          if (x >= E2.nbelow && x < E2.nbelow + n) {
            const int i = x - E2.nbelow;
            for (int64_t k = P.ia[(size_t)i]; k < P.ia[(size_t)i + 1]; k++)
              if (P.gj[(size_t)k] >= cs && P.gj[(size_t)k] < cs + ncl) f((int)(P.gj[(size_t)k] - cs), x, P.a[(size_t)k]);
          } else {
            const Incoming &in = inc_of(x);
            for (size_t k = 0; k < in.pc.size(); k++) f((int)(in.pc[k] - cs), x, in.pv[k]);
          }
        }
      };
      each_entry([&](int r, int, double) { Re.ia[(size_t)r + 1]++; });
      for (int r = 0; r < ncl; r++) Re.ia[(size_t)r + 1] += Re.ia[(size_t)r];
      Re.ja.resize((size_t)Re.nnz());
      Re.a.resize((size_t)Re.nnz());
      {
        std::vector<int64_t> pos(Re.ia.begin(), Re.ia.end() - 1);
        each_entry([&](int r, int x, double v) {
          Re.ja[(size_t)pos[(size_t)r]] = x;
          Re.a[(size_t)pos[(size_t)r]++] = v;
        });
      }
      lap("galerkin: R = P^T");
      HostCSR Ace;
      spgemm_auto(Re, APe, Ace, device_min_rows);
      lap("galerkin: R*(A*P)");
      GlobCSR &Ac = Ln.A;
      Ac.nrows = ncl;
      Ac.ia = Ace.ia;
      Ac.a.swap(Ace.a);
      Ac.gj.resize(Ace.ja.size());
      parallel_for((int64_t)Ace.ja.size(), [&](int64_t b, int64_t en, int) {
        for (int64_t k = b; k < en; k++) Ac.gj[(size_t)k] = CE2.global(Ace.ja[(size_t)k]);
      });
      if (p.non_galerkin_tol_for(l) > 0.0) sparsify_non_galerkin_dist(comm, Ac, Ln.starts, p.non_galerkin_tol_for(l));
      GlobCSR &R = Lv.R;
      R.nrows = ncl;
      R.ia = Re.ia;
      R.a.swap(Re.a);
      R.gj.resize(Re.ja.size());
      parallel_for((int64_t)Re.ja.size(), [&](int64_t b, int64_t en, int) {
        for (int64_t k = b; k < en; k++) R.gj[(size_t)k] = E2.global(Re.ja[(size_t)k]);
      });
      lap("galerkin: results to global ids");
    }
    t_phase[3] += wall_time() - tp0;
    l++;
  }
  // a level below the threshold is redundant also when the coarsening ended on it (see build_replicated)
  if (!has_tail && red_rows > 0 && D.size() >= 2 && D.back().starts.back() <= red_rows) has_tail = true;
  const size_t nlev = D.size();

  // ---- C-first ordering of every level with a splitting, and the final ParCSR blocks
  tp0 = wall_time();
  tsub = tp0;
  std::vector<std::vector<int>> pos(nlev), perm(nlev);
  for (size_t li = 0; li < nlev; li++) {
    const DLevel &Lv = D[li];
    if (!Lv.has_cf) continue;
    const int n = (int)Lv.cf.size();  // (the operator of a device-built level is not in Lv.A)
    pos[li].resize((size_t)n), perm[li].resize((size_t)n);
    // C points first, both groups in their old order: per-block counts, then every block places its own rows
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (int64_t)n / 65536 + 1));
    const int64_t per = ((int64_t)n + nblk - 1) / nblk;
    std::vector<int64_t> cnt_c((size_t)nblk + 1, 0);
    parallel_for(nblk, [&](int64_t b, int64_t e, int) {
      for (int64_t t = b; t < e; t++) {
        int64_t c = 0;
        for (int64_t i = t * per; i < std::min<int64_t>(n, (t + 1) * per); i++) c += (Lv.cf[(size_t)i] == C_PT);
        cnt_c[(size_t)t + 1] = c;
      }
    });
    for (int t = 0; t < nblk; t++) cnt_c[(size_t)t + 1] += cnt_c[(size_t)t];
    const int64_t nc_all = cnt_c[(size_t)nblk];
    std::vector<int> &ps = pos[li], &pm = perm[li];
    parallel_for(nblk, [&](int64_t b, int64_t e, int) {
      for (int64_t t = b; t < e; t++) {
        int64_t qc = cnt_c[(size_t)t], qf = nc_all + (t * per - cnt_c[(size_t)t]);
        for (int64_t i = t * per; i < std::min<int64_t>(n, (t + 1) * per); i++) {
          const int64_t q = (Lv.cf[(size_t)i] == C_PT) ? qc++ : qf++;
          ps[(size_t)i] = (int)q;
          pm[(size_t)q] = (int)i;
        }
      }
    });
  }
  lap("ordering: C-first positions");
  // new global ids of the columns of M (ids of level `lev`)
  auto translate = [&](const GlobCSR &M, size_t lev, const Ring *known_ring) {
    std::vector<gidx> out(M.gj);
    // (by the level's state, not by this rank's row count: a rank without rows on the level still takes part in the
    // exchanges below)
    if (!D[lev].has_cf) return out;
    const std::vector<gidx> &st = D[lev].starts;
    const gidx s = st[(size_t)rank], e = st[(size_t)rank + 1];
    Ring own;
    const Ring *rg = known_ring;
    if (!rg) {
      std::vector<gidx> need;
      for (gidx g : M.gj)
        if (g < s || g >= e) need.push_back(g);
      sort_unique(need);
      own.build(comm, st, std::move(need));
      rg = &own;
    }
    const std::vector<int> pos_h = rg->forward(comm, pos[lev]);
    parallel_for((int64_t)out.size(), [&](int64_t b, int64_t en, int) {
      for (int64_t k = b; k < en; k++) {
        const gidx g = M.gj[(size_t)k];
        if (g >= s && g < e)
          out[(size_t)k] = s + pos[lev][(size_t)(g - s)];
        else
          out[(size_t)k] = st[(size_t)rank_of_id(st, g)] + pos_h[(size_t)rg->slot_of(g)];
      }
    });
    return out;
  };
  L.clear();
  L.resize(nlev);
  tail.reset();
  tail_A.reset();
  // new global ids of the remote ids `ids` of level `lev` after its C-first renumbering (ring: over exactly these ids)
  auto new_ids = [&](const std::vector<gidx> &ids, size_t lev, const Ring &rg) {
    std::vector<gidx> out(ids);
    if (!D[lev].has_cf) return out;
    const std::vector<gidx> &st = D[lev].starts;
    const std::vector<int> pos_h = rg.forward(comm, pos[lev]);
    for (size_t k = 0; k < ids.size(); k++) out[k] = st[(size_t)rank_of_id(st, ids[k])] + pos_h[k];
    return out;
  };
  for (size_t li = 0; li < nlev; li++) {
    DLevel &Lv = D[li];
    AmgLevel &Out = L[li];
    if ((int)li < n_dev_levels) {
      // a level that was built on the device: renumbered, split and kept there (Out.oA / oP / oR)
      hipStream_t s = ctx().stream;
      DevLevel &V = DB.lev[li];
      const int n = (int)Lv.cf.size();
      const std::vector<gidx> &cst = D[li + 1].starts;
      Out.A_own = assemble_dev(V.A, V.E, perm[li], pos[li], new_ids(V.E.remote, li, V.ring1), Lv.starts, Lv.starts, rank, Out.oA, s);
      V.A.release();
      lap("ordering: device A");
      Out.A = Out.A_own.get();
      Out.A->build_halo_plan(comm);
      Out.has_cf = true;
      Out.perm = perm[li];
      std::vector<int> &ocf = Out.cf.hostw();
      ocf.resize((size_t)n);
      {
        std::atomic<long long> ncs{0};
        parallel_for(n, [&](int64_t b, int64_t e, int) {
          long long c = 0;
          for (int64_t q = b; q < e; q++) {
            ocf[(size_t)q] = Lv.cf[(size_t)perm[li][(size_t)q]];
            c += (ocf[(size_t)q] == C_PT);
          }
          ncs += c;
        });
        Out.nc = (int)ncs.load();
      }
      lap("ordering: cf");
      {
        Ring rp;
        rp.build(comm, cst, V.CE.remote);
        Out.Pm = assemble_dev(V.P, V.CE, perm[li], pos[li + 1], new_ids(V.CE.remote, li + 1, rp), Lv.starts, cst, rank, Out.oP, s);
        V.P.release();
      }
      if (!(has_tail && li + 2 == nlev)) Out.Pm->build_halo_plan(comm);
      lap("ordering: device P");
      {
        Ring rr;
        rr.build(comm, Lv.starts, V.E2.remote);
        Out.Rm = assemble_dev(V.R, V.E2, perm[li + 1], pos[li], new_ids(V.E2.remote, li, rr), cst, Lv.starts, rank, Out.oR, s);
        V.R.release();
      }
      Out.Rm->build_halo_plan(comm);
      lap("ordering: device R");
      continue;
    }
    const int n = Lv.A.nrows;
    const bool ring_ok = Lv.has_cf;  // the halo ring of A was built in the coarsening loop
    std::vector<gidx> newcol_a = translate(Lv.A, li, ring_ok ? &Lv.ring : nullptr);
    lap("ordering: translate A");
    Out.A_own = assemble_rows(Lv.A, perm[li], newcol_a, Lv.starts, Lv.starts, rank);
    std::vector<gidx>().swap(newcol_a);
    lap("ordering: assemble A");
    Out.A = Out.A_own.get();
    Out.A->build_halo_plan(comm);
    lap("ordering: halo plans");
    Out.has_cf = Lv.has_cf;
    if (Lv.has_cf) {
      Out.perm = perm[li];
      std::vector<int> &ocf = Out.cf.hostw();
      ocf.resize((size_t)n);
      Out.nc = 0;
      for (int q = 0; q < n; q++) {
        ocf[(size_t)q] = Lv.cf[(size_t)perm[li][(size_t)q]];
        Out.nc += (ocf[(size_t)q] == C_PT);
      }
      lap("ordering: cf");
      std::vector<gidx> newcol_p = translate(Lv.P, li + 1, nullptr);
      lap("ordering: translate P");
      Out.Pm = assemble_rows(Lv.P, perm[li], newcol_p, Lv.starts, D[li + 1].starts, rank);
      std::vector<gidx>().swap(newcol_p);
      lap("ordering: assemble P");
      // with a redundant tail the coarse correction is whole on every rank: no exchange for the last P
      if (!(has_tail && li + 2 == nlev)) Out.Pm->build_halo_plan(comm);
      lap("ordering: halo plans");
      std::vector<gidx> newcol_r = translate(Lv.R, li, nullptr);
      lap("ordering: translate R");
      Out.Rm = assemble_rows(Lv.R, perm[li + 1], newcol_r, D[li + 1].starts, Lv.starts, rank);
      std::vector<gidx>().swap(newcol_r);
      lap("ordering: assemble R");
      Out.Rm->build_halo_plan(comm);
      lap("ordering: halo plans");
    }
  }
  if (!order_h.empty()) {  // level-0 rows -> caller rows
    AmgLevel &L0 = L[0];
    if (L0.perm.empty()) {
      L0.perm = order_h;
    } else {
      for (int &q : L0.perm.hostw()) q = order_h[(size_t)q];
    }
    input_order = std::move(order_h);
  }
  lap("ordering: rest");
  if (has_tail) {
    // the first redundant level: gathered once, then one single-rank hierarchy per rank (as before)
    const DLevel &Ls = D[nlev - 1];
    const gidx Ng = Ls.starts.back();
    MI_REQUIRE(Ng < (gidx)2147483000, "redundant level exceeds int32");
    g_global_rows_gathered += Ng;
    std::vector<char> mine;
    {
      const GlobCSR &G = Ls.A;
      std::vector<int> len((size_t)G.nrows);
      for (int i = 0; i < G.nrows; i++) len[(size_t)i] = (int)(G.ia[(size_t)i + 1] - G.ia[(size_t)i]);
      put(mine, len.data(), len.size());
      put(mine, G.gj.data(), G.gj.size());
      put(mine, G.a.data(), G.a.size());
    }
    std::vector<size_t> offs;
    std::vector<char> everyone;
    comm.allgatherv_host(mine.data(), mine.size(), offs, everyone);
    tail_A.reset(new ParCSR());
    HostCSR &G = tail_A->diag;
    G.nrows = G.ncols = (int)Ng;
    G.ia.assign((size_t)Ng + 1, 0);
    for (int r = 0; r < size; r++) {
      const gidx rs = Ls.starts[(size_t)r], re = Ls.starts[(size_t)r + 1];
      const int *len = reinterpret_cast<const int *>(everyone.data() + offs[(size_t)r]);
      for (gidx g = rs; g < re; g++) G.ia[(size_t)g + 1] = G.ia[(size_t)g] + len[(size_t)(g - rs)];
    }
    G.ja.resize((size_t)G.nnz());
    G.a.resize((size_t)G.nnz());
    for (int r = 0; r < size; r++) {
      const gidx rs = Ls.starts[(size_t)r], re = Ls.starts[(size_t)r + 1];
      if (re == rs) continue;
      const size_t nr = (size_t)(re - rs), tot = (size_t)(G.ia[(size_t)re] - G.ia[(size_t)rs]);
      const char *base = everyone.data() + offs[(size_t)r] + sizeof(int) * nr;
      std::vector<gidx> cols(tot);
      memcpy(cols.data(), base, tot * sizeof(gidx));
      for (size_t k = 0; k < tot; k++) G.ja[(size_t)G.ia[(size_t)rs] + k] = (int)cols[k];
      memcpy(G.a.data() + G.ia[(size_t)rs], base + tot * sizeof(gidx), tot * sizeof(double));
    }
    tail_A->nrows = (int)Ng;
    tail_A->row_start = 0;
    tail_A->row_end = Ng;
    tail_A->row_starts = {0, Ng};
    tail_A->offd.nrows = (int)Ng;
    tail_A->offd.ncols = 0;
    tail_A->offd.ia.assign((size_t)Ng + 1, 0);
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
    tail_start = Ls.starts[(size_t)rank];
    int slot = 0;
    for (int r = 0; r < size; r++) slot = std::max(slot, (int)(Ls.starts[(size_t)r + 1] - Ls.starts[(size_t)r]));
    tail_slot = slot;
    std::vector<int> map((size_t)Ng);
    for (int r = 0; r < size; r++)
      for (gidx i = Ls.starts[(size_t)r]; i < Ls.starts[(size_t)r + 1]; i++) map[(size_t)i] = r * slot + (int)(i - Ls.starts[(size_t)r]);
    tail_map_host.swap(map);
  }
  t_phase[4] += wall_time() - tp0;
  if (sub_timing)
    for (auto &kv : sub_times) printf("   distributed setup, %-40s %.2f s\n", kv.first.c_str(), kv.second);
  if (p.print_level > 0 && rank == 0)
    printf("mi_hypre BoomerAMG: distributed setup on %d ranks (%zu distributed levels%s; largest per-rank sub-problem %lld "
           "rows of %lld global)\n",
           size, nlev, has_tail ? " + redundant tail" : "", g_ext_rows_max, (long long)A0.global_rows());
}

}  // namespace mi
