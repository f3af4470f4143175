// Opt-in adapter: the SAME driver (HypreSystem + main) built against a real libHYPRE instead of libmi_hypre.so
//   make -C hypre-mini-app_amd app-libhypre HYPRE_DIR=/path/to/hypre/install [MPICXX=mpicxx]
// (SURVEY.md 8c last row).  libHYPRE is not in this image, so this configuration cannot be
// built or run here; it exists so that, where a CPU libHYPRE is available, the reference-HYPRE iteration counts
// and timings can be put beside this library's on identical inputs.  Nothing here stands in for HYPRE: with
// MI_HOST_WITH_LIBHYPRE every HYPRE_* symbol comes from $(HYPRE_DIR).
#pragma once
#ifdef MI_HOST_WITH_LIBHYPRE
#include <mpi.h>

#include <cstdlib>
#include <vector>

inline int mi_env_int(const char *name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }

// the synthetic generator the driver otherwise takes from the library (HYPRE_MI_Laplace3D): global rows
// [ilower, iupper] of the nx*ny*nz grid, lexicographic numbering, 7-pt (6 / -1) or 27-pt (26 / -1), rhs = row sum
inline int HYPRE_MI_Laplace3D(int nx, int ny, int nz, int stencil, HYPRE_BigInt ilower, HYPRE_BigInt iupper,
                              HYPRE_BigInt *nnz, HYPRE_BigInt **rows, HYPRE_BigInt **cols, HYPRE_Complex **vals,
                              HYPRE_Complex **rhs) {
  std::vector<HYPRE_BigInt> r, c;
  std::vector<HYPRE_Complex> v, b;
  const double dv = stencil == 27 ? 26.0 : 6.0;
  for (HYPRE_BigInt row = ilower; row <= iupper; row++) {
    const int x = (int)(row % nx), y = (int)((row / nx) % ny), z = (int)(row / ((HYPRE_BigInt)nx * ny));
    double sum = 0.0;
    for (int dz = -1; dz <= 1; dz++)
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          if (stencil == 7 && abs(dx) + abs(dy) + abs(dz) > 1) continue;
          const int X = x + dx, Y = y + dy, Z = z + dz;
          if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
          const HYPRE_BigInt col = X + (HYPRE_BigInt)nx * (Y + (HYPRE_BigInt)ny * Z);
          r.push_back(row), c.push_back(col), v.push_back(col == row ? dv : -1.0);
          sum += v.back();
        }
    b.push_back(sum);
  }
  *nnz = (HYPRE_BigInt)v.size();
  *rows = (HYPRE_BigInt *)malloc(sizeof(HYPRE_BigInt) * (r.size() + 1));
  *cols = (HYPRE_BigInt *)malloc(sizeof(HYPRE_BigInt) * (c.size() + 1));
  *vals = (HYPRE_Complex *)malloc(sizeof(HYPRE_Complex) * (v.size() + 1));
  *rhs = (HYPRE_Complex *)malloc(sizeof(HYPRE_Complex) * (b.size() + 1));
  std::copy(r.begin(), r.end(), *rows), std::copy(c.begin(), c.end(), *cols);
  std::copy(v.begin(), v.end(), *vals), std::copy(b.begin(), b.end(), *rhs);
  return 0;
}
inline void HYPRE_MI_Free(void *p) { free(p); }
// the same arrays in libHYPRE's device memory space (linear_system: mi_device_assembly; host memory in a CPU build)
inline int HYPRE_MI_Laplace3DDevice(int nx, int ny, int nz, int stencil, HYPRE_BigInt ilower, HYPRE_BigInt iupper,
                                    HYPRE_BigInt *nnz, HYPRE_BigInt **rows, HYPRE_BigInt **cols, HYPRE_Complex **vals,
                                    HYPRE_Complex **rhs) {
  // (never compiled where this was written -- no libHYPRE there; whoever builds app-libhypre first: check it)
  HYPRE_BigInt *r = nullptr, *c = nullptr;
  HYPRE_Complex *v = nullptr, *b = nullptr;
  const int rc = HYPRE_MI_Laplace3D(nx, ny, nz, stencil, ilower, iupper, nnz, &r, &c, &v, &b);
  if (rc || !r || !c || !v || !b) {
    free(r), free(c), free(v), free(b);
    return rc ? rc : 1;
  }
  const size_t ne = (size_t)*nnz + 1, nr = (size_t)(iupper - ilower + 1) + 1;
  *rows = hypre_TAlloc(HYPRE_BigInt, ne, HYPRE_MEMORY_DEVICE);
  *cols = hypre_TAlloc(HYPRE_BigInt, ne, HYPRE_MEMORY_DEVICE);
  *vals = hypre_TAlloc(HYPRE_Complex, ne, HYPRE_MEMORY_DEVICE);
  *rhs = hypre_TAlloc(HYPRE_Complex, nr, HYPRE_MEMORY_DEVICE);
  if (!*rows || !*cols || !*vals || !*rhs) {
    hypre_Free(*rows, HYPRE_MEMORY_DEVICE), hypre_Free(*cols, HYPRE_MEMORY_DEVICE);
    hypre_Free(*vals, HYPRE_MEMORY_DEVICE), hypre_Free(*rhs, HYPRE_MEMORY_DEVICE);
    free(r), free(c), free(v), free(b);
    return 2;
  }
  hypre_TMemcpy(*rows, r, HYPRE_BigInt, ne - 1, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
  hypre_TMemcpy(*cols, c, HYPRE_BigInt, ne - 1, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
  hypre_TMemcpy(*vals, v, HYPRE_Complex, ne - 1, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
  hypre_TMemcpy(*rhs, b, HYPRE_Complex, nr - 1, HYPRE_MEMORY_DEVICE, HYPRE_MEMORY_HOST);
  free(r), free(c), free(v), free(b);
  return 0;
}
inline void HYPRE_MI_FreeDevice(void *p) { hypre_Free(p, HYPRE_MEMORY_DEVICE); }
#endif
