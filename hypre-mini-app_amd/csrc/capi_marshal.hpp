// Caller arrays <-> HostCSR for the ...Op test hooks of capi.cpp (HYPRE_MI_CSRReuseOp, MMInterpOp, AIRRestrictionOp,
// FSAIAdaptiveOp, OnePointInterpOp, CSRDeviceOp): one checked copy-in, one malloc'ed copy-out, and the two argument
// checks the hooks share.  Host code only; profiles/debug/capi_marshal_asan_main.cpp runs it under the sanitizers.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

#include "HYPRE_utilities.h"
#include "mi_internal.hpp"

namespace mi {

// caller arrays of an nrows x ncols CSR, checked: ia[0] == 0, row pointers that do not decrease, columns in range and
// strictly ascending within a row.  ja may be NULL when there are no entries; a == NULL: a pattern, values 0.
inline HostCSR csr_of(const std::string &who, const char *what, HYPRE_Int nrows, HYPRE_Int ncols, const HYPRE_BigInt *ia,
                      const HYPRE_Int *ja, const HYPRE_Complex *a) {
  if (nrows < 0 || ncols < 0 || !ia || ia[0] != 0) fail(HYPRE_ERROR_ARG, who + ": bad dimensions of " + what);
  HostCSR h;
  h.nrows = nrows;
  h.ncols = ncols;
  h.ia.assign(ia, ia + nrows + 1);
  for (HYPRE_Int i = 0; i < nrows; i++)
    if (ia[i + 1] < ia[i]) fail(HYPRE_ERROR_ARG, who + ": row pointers of " + what + " decrease");
  const HYPRE_BigInt nnz = ia[nrows];
  if (nnz > 0 && !ja) fail(HYPRE_ERROR_ARG, who + ": NULL columns of " + what);
  for (HYPRE_Int i = 0; i < nrows; i++)
    for (HYPRE_BigInt k = ia[i]; k < ia[i + 1]; k++)
      if (ja[k] < 0 || ja[k] >= ncols || (k > ia[i] && ja[k] <= ja[k - 1]))
        fail(HYPRE_ERROR_ARG, who + ": columns of " + what + " out of range or not ascending");
  if (nnz > 0) h.ja.assign(ja, ja + nnz);
  if (nnz > 0 && a)
    h.a.assign(a, a + nnz);
  else
    h.a.assign((size_t)nnz, 0.0);
  return h;
}

// a HostCSR of nrows rows as malloc'ed caller arrays (HYPRE_MI_Free); a matrix nobody built (no row pointers) has none
inline void csr_to_caller(const HostCSR &h, int nrows, HYPRE_BigInt **ia, HYPRE_Int **ja, HYPRE_Complex **a) {
  *ia = (HYPRE_BigInt *)malloc(sizeof(HYPRE_BigInt) * ((size_t)nrows + 1));
  *ja = (HYPRE_Int *)malloc(sizeof(HYPRE_Int) * std::max<size_t>(1, h.ja.size()));
  *a = (HYPRE_Complex *)malloc(sizeof(HYPRE_Complex) * std::max<size_t>(1, h.a.size()));
  (*ia)[0] = 0;
  for (int i = 1; i <= nrows; i++) (*ia)[i] = h.ia.empty() ? 0 : h.ia[(size_t)i];
  if (!h.ja.empty()) {
    memcpy(*ja, h.ja.data(), h.ja.size() * sizeof(int));
    memcpy(*a, h.a.data(), h.a.size() * sizeof(double));
  }
}

// a C/F marker of n entries: +1 C, -1 F and, where the routine knows it, -3 special F.  Returns the number of C points.
inline int check_marker(const std::string &who, const HYPRE_Int *cf, HYPRE_Int n, bool special_f) {
  if (n > 0 && !cf) fail(HYPRE_ERROR_ARG, who + ": NULL marker");
  int nc = 0;
  for (HYPRE_Int i = 0; i < n; i++) {
    if (cf[i] != 1 && cf[i] != -1 && !(special_f && cf[i] == -3))
      fail(HYPRE_ERROR_ARG, who + ": the marker holds a value other than 1, -1" + (special_f ? ", -3" : ""));
    nc += cf[i] == 1;
  }
  return nc;
}

// lanes per row of a kernel: 0 = the library's choice, or a power of two up to 64
inline void check_lanes(const std::string &who, HYPRE_Int lanes) {
  if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) fail(HYPRE_ERROR_ARG, who + ": lanes must be 0 or a power of two up to 64");
}

}  // namespace mi
