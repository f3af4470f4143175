// The caller-array marshalling of the ...Op test hooks (csrc/capi_marshal.hpp: csr_of, csr_to_caller, check_marker,
// check_lanes) under AddressSanitizer + UBSan, as a stand-alone program without a GPU:
//   cd hypre-mini-app_amd
//   hipcc -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
//     ../profiles/debug/capi_marshal_asan_main.cpp -o ../profiles/debug/capi_marshal_asan
//   UBSAN_OPTIONS=halt_on_error=1 ../profiles/debug/capi_marshal_asan
// Every array is a heap block of exactly the promised size, so a read or write past it is reported.
#include <cstdio>
#include <memory>
#include <vector>

#include "capi_marshal.hpp"

using namespace mi;

namespace {

int failures = 0;

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}

struct Case {
  const char *name;
  HYPRE_Int nrows, ncols;
  std::vector<HYPRE_BigInt> ia;
  std::vector<HYPRE_Int> ja;
  bool null_ja, null_a;
  const char *refusal;  // words of the expected message, or null: accepted
};

void run(const Case &c) {
  auto ia = exact(c.ia);
  auto ja = exact(c.ja);
  std::vector<HYPRE_Complex> vals(c.ja.size());
  for (size_t k = 0; k < vals.size(); k++) vals[k] = 1.0 + (double)k;
  auto a = exact(vals);
  std::string got;
  try {
    const HostCSR h = csr_of("Op", "A", c.nrows, c.ncols, c.ia.empty() ? nullptr : ia.get(), c.null_ja ? nullptr : ja.get(),
                             c.null_a ? nullptr : a.get());
    bool same = h.nrows == c.nrows && h.ncols == c.ncols && h.ia.size() == c.ia.size() && h.ja.size() == c.ja.size() &&
                h.a.size() == c.ja.size();
    for (size_t k = 0; same && k < c.ja.size(); k++) same = h.ja[k] == c.ja[k] && h.a[k] == (c.null_a ? 0.0 : vals[k]);
    HYPRE_BigInt *oia = nullptr;
    HYPRE_Int *oja = nullptr;
    HYPRE_Complex *oa = nullptr;
    csr_to_caller(h, c.nrows, &oia, &oja, &oa);
    for (size_t i = 0; same && i < c.ia.size(); i++) same = oia[i] == c.ia[i];
    for (size_t k = 0; same && k < c.ja.size(); k++) same = oja[k] == c.ja[k] && oa[k] == h.a[k];
    free(oia), free(oja), free(oa);
    if (!same) got = "(accepted, but the round trip differs)";
  } catch (const Error &e) {
    got = e.what();
    if (e.code != HYPRE_ERROR_ARG) got += " (not HYPRE_ERROR_ARG)";
  }
  const bool ok = c.refusal ? (got.find(c.refusal) != std::string::npos && got.find("not HYPRE_ERROR_ARG") == std::string::npos)
                            : got.empty();
  if (!ok) failures++;
  printf("%-44s %s%s%s\n", c.name, ok ? "ok" : "FAIL", got.empty() ? "" : ": ", got.c_str());
}

void refused(const char *name, const char *words, void (*f)()) {
  std::string got;
  try {
    f();
  } catch (const Error &e) {
    got = e.what();
  }
  const bool ok = words ? got.find(words) != std::string::npos : got.empty();
  if (!ok) failures++;
  printf("%-44s %s%s%s\n", name, ok ? "ok" : "FAIL", got.empty() ? "" : ": ", got.c_str());
}

}  // namespace

int main() {
  const std::vector<Case> cases = {
      {"0 x 0, every array empty", 0, 0, {0}, {}, false, false, nullptr},
      {"0 x 0, NULL ja and a", 0, 0, {0}, {}, true, true, nullptr},
      {"zero rows, 5 columns", 0, 5, {0}, {}, true, true, nullptr},
      {"3 x 0 without entries", 3, 0, {0, 0, 0, 0}, {}, true, false, nullptr},
      {"3 x 4 without entries, NULL ja", 3, 4, {0, 0, 0, 0}, {}, true, true, nullptr},
      {"3 x 4 with an empty row", 3, 4, {0, 2, 2, 4}, {0, 3, 1, 2}, false, false, nullptr},
      {"3 x 4 as a pattern (NULL a)", 3, 4, {0, 2, 2, 4}, {0, 3, 1, 2}, false, true, nullptr},
      {"1 x 1", 1, 1, {0, 1}, {0}, false, false, nullptr},
      {"NULL ia", 2, 2, {}, {}, true, true, "bad dimensions of A"},
      {"negative rows", -1, 2, {0}, {}, true, true, "bad dimensions of A"},
      {"negative columns", 1, -1, {0, 0}, {}, true, true, "bad dimensions of A"},
      {"ia[0] != 0", 2, 2, {1, 1, 2}, {0, 1}, false, false, "bad dimensions of A"},
      {"row pointers decrease", 3, 3, {0, 2, 1, 3}, {0, 1, 2}, false, false, "row pointers of A decrease"},
      {"row pointers decrease below zero", 2, 3, {0, -1, 0}, {}, true, true, "row pointers of A decrease"},
      {"entries but NULL ja", 2, 2, {0, 1, 2}, {0, 1}, true, false, "NULL columns of A"},
      {"column below zero", 2, 2, {0, 1, 2}, {-1, 1}, false, false, "out of range or not ascending"},
      {"column == ncols", 2, 2, {0, 1, 2}, {0, 2}, false, false, "out of range or not ascending"},
      {"columns descend in a row", 2, 3, {0, 2, 3}, {2, 1, 0}, false, false, "out of range or not ascending"},
      {"a column twice in a row", 2, 3, {0, 2, 3}, {1, 1, 0}, false, false, "out of range or not ascending"},
      {"a column of a 3 x 0 matrix", 3, 0, {0, 0, 1, 1}, {0}, false, false, "out of range or not ascending"},
  };
  for (const Case &c : cases) run(c);

  // csr_to_caller of a matrix nobody built (MMInterpOp with n = 0)
  {
    HYPRE_BigInt *oia = nullptr;
    HYPRE_Int *oja = nullptr;
    HYPRE_Complex *oa = nullptr;
    csr_to_caller(HostCSR(), 0, &oia, &oja, &oa);
    const bool ok = oia && oja && oa && oia[0] == 0;
    if (!ok) failures++;
    printf("%-44s %s\n", "copy-out of an unbuilt 0-row matrix", ok ? "ok" : "FAIL");
    free(oia), free(oja), free(oa);
  }

  refused("marker 1, -1", nullptr, [] {
    const auto m = exact(std::vector<HYPRE_Int>{1, -1, -1, 1});
    if (check_marker("Op", m.get(), 4, false) != 2) fail(1, "wrong C count");
  });
  refused("marker with -3 where it is known", nullptr, [] {
    const auto m = exact(std::vector<HYPRE_Int>{1, -3, -1});
    if (check_marker("Op", m.get(), 3, true) != 1) fail(1, "wrong C count");
  });
  refused("marker with -3 where it is not", "other than 1, -1", [] {
    const auto m = exact(std::vector<HYPRE_Int>{1, -3, -1});
    check_marker("Op", m.get(), 3, false);
  });
  refused("marker with 0", "other than 1, -1, -3", [] {
    const auto m = exact(std::vector<HYPRE_Int>{1, 0});
    check_marker("Op", m.get(), 2, true);
  });
  refused("NULL marker of 2 entries", "NULL marker", [] { check_marker("Op", nullptr, 2, true); });
  refused("NULL marker of no entries", nullptr, [] { check_marker("Op", nullptr, 0, true); });
  refused("lanes 0, 1, 2, ... 64", nullptr, [] {
    for (HYPRE_Int lanes : {0, 1, 2, 4, 8, 16, 32, 64}) check_lanes("Op", lanes);
  });
  refused("lanes 3", "lanes must be", [] { check_lanes("Op", 3); });
  refused("lanes 128", "lanes must be", [] { check_lanes("Op", 128); });
  refused("lanes -2", "lanes must be", [] { check_lanes("Op", -2); });

  printf(failures ? "FAIL: %d case(s)\n" : "all cases ok\n", failures);
  return failures ? 1 : 0;
}
