// The host path of an IJ update round (parcsr.cpp: assemble_parcsr, check_update_batch, update_parcsr_values) under
// AddressSanitizer + UBSan, as a stand-alone program without a GPU:
//   cd hypre-mini-app_amd && make && mkdir -p build_asan
//   S="-O1 -g -std=c++17 -fPIC -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc"
//   hipcc $S -c ../profiles/debug/ij_update_asan_main.cpp -o build_asan/ij_update_asan_main.o
//   hipcc $S -c csrc/parcsr.cpp -o build_asan/parcsr_upd.o
//   hipcc -fsanitize=address,undefined --offload-arch=gfx950 build_asan/ij_update_asan_main.o build_asan/parcsr_upd.o \
//     $(ls build/*.o | grep -v parcsr.o) -ldl -pthread -o ../profiles/debug/ij_update_asan
//   UBSAN_OPTIONS=halt_on_error=1 ../profiles/debug/ij_update_asan
#include <cstdio>
#include <random>

#include "parcsr.hpp"

using namespace mi;

static IJEntryBatch batch(std::mt19937 &rng, const std::vector<std::pair<gidx, gidx>> &pairs, size_t n, bool add) {
  IJEntryBatch b;
  b.add = add;
  for (size_t k = 0; k < n; k++) {
    const auto &p = pairs[rng() % pairs.size()];
    b.rows.push_back(p.first);
    b.cols.push_back(p.second);
    b.vals.push_back((double)(rng() % 1000) / 7.0);
  }
  return b;
}

int main() {
  const int n = 500;
  std::mt19937 rng(7);
  std::vector<std::pair<gidx, gidx>> pairs;
  for (int r = 0; r < n; r++) {
    if (r % 50 == 17) continue;  // empty rows
    for (int k = 0, len = 1 + (int)(rng() % 9); k < len; k++) pairs.push_back({r, (gidx)(rng() % n)});
  }
  Comm &comm = current_comm();
  std::vector<IJEntryBatch> first;
  first.push_back(batch(rng, pairs, 0, false));
  for (auto &p : pairs) first[0].rows.push_back(p.first), first[0].cols.push_back(p.second), first[0].vals.push_back(1.0);
  ParCSR A;
  assemble_parcsr(comm, 0, n - 1, 0, n - 1, first, A);
  const unsigned long long stamp = A.assembly_stamp;
  std::vector<IJEntryBatch> round;
  round.push_back(batch(rng, pairs, 3000, true));
  round.push_back(batch(rng, pairs, 0, false));  // an empty batch
  round.push_back(batch(rng, pairs, 2000, false));
  std::vector<IJUpdateConst> consts = {{0, 0.0}, {2, 2.5}, {3, -1.0}, {7, 4.0}};  // also one past the last batch
  update_parcsr_values(A, 0, n - 1, round, consts);
  for (double v : A.diag.a)
    if (v != 4.0) return printf("FAIL: a constant as the last call must win\n"), 1;
  consts.resize(2);
  update_parcsr_values(A, 0, n - 1, round, consts);
  int refused = 0;
  for (auto bad : {std::pair<gidx, gidx>{3, n + 4}, {n + 1, 2}, {-5, 2}, {17, 3}}) {
    IJEntryBatch b = batch(rng, pairs, 100, true);
    b.rows.push_back(bad.first), b.cols.push_back(bad.second), b.vals.push_back(1.0);
    try {
      check_update_batch(A, 0, n - 1, b);
    } catch (const Error &e) {
      refused++;
    }
    try {
      std::vector<IJEntryBatch> r2 = {b};
      update_parcsr_values(A, 0, n - 1, r2, {});
    } catch (const Error &e) {
      refused++;
    }
  }
  if (refused != 8 || A.assembly_stamp == stamp) return printf("FAIL: %d refusals\n", refused), 1;
  printf("ij update host path ok: %lld entries, %d refusals\n", (long long)A.diag.nnz(), refused);
  return 0;
}
