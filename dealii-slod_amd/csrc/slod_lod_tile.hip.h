// The tiling of the kernels on coarse multi-vectors (interleaved [row][column], columns on lanes):
// columns in chunks of LOD_COLS (blockIdx.y), a block takes groups of LOD_ROWS consecutive rows of one chunk (group
// blockIdx.x, += gridDim.x) and spreads the (row, column) items of a group over its LOD_BLOCK threads, row-major.  The row
// product, the sum over the rows of a group and the sum over the groups are defined here once, each in ascending order
// whatever n_rhs, the column's position or ld: the bits of a column depend on the matrix and that column only.
#ifndef SLOD_LOD_TILE_HIP_H
#define SLOD_LOD_TILE_HIP_H
#include "slod_host.h"

namespace
{
  constexpr int LOD_COLS  = 64;  // columns per chunk (one wave wide)
  constexpr int LOD_ROWS  = 16;  // rows per reduction group: every summation order hangs on it
  constexpr int LOD_BLOCK = 256; // threads per block

  // The launch shape of these kernels for n_rhs columns on the block rows of a handle.
  struct LodShape
  {
    int s, cap, NP, nrow, ngroup, nchunk;
  };
  inline LodShape lod_shape(const slod_handle *h, int n_rhs)
  {
    const int s = h->cfg.spacedim, nrow = h->NP * s;
    return {s, slod_lod_row_capacity(h), h->NP, nrow, (nrow + LOD_ROWS - 1) / LOD_ROWS, (n_rhs + LOD_COLS - 1) / LOD_COLS};
  }
  // at most max_blocks blocks per chunk (a block walks several groups beyond that); nz: blockIdx.z
  inline dim3 lod_grid(const LodShape &w, int max_blocks, int nz = 1)
  {
    return dim3((unsigned)std::min(w.ngroup, max_blocks), (unsigned)w.nchunk, (unsigned)nz);
  }
  // one thread per element of a flat array of n
  inline dim3 lod_flat_grid(size_t n) { return dim3((unsigned)((n + LOD_BLOCK - 1) / LOD_BLOCK)); }
} // namespace

// sum_j sum_e values[(p cap + j) s s + d s + e] x[(cols[p cap + j] s + e) ld + col] for row i = p s + d: one fma chain
// over the slots of the row in ascending order.
// PER_COL: a matrix per column on the one pattern (the ensemble layout of include/slod.h), entry e of column col's matrix
// at values[e ld_m + col].  The chain is the same, on other operands; the lanes of a wave, which hold consecutive columns
// of one row, read 64 consecutive words where the shared matrix gives them one.  There every (row, column) streams its
// own values, so the loads of LOD_SLOTS slots are issued before the first fma needs one (they do not depend on acc): a
// wave otherwise waits out a memory latency per slot.  mcol: the column of the matrix, col: that of the vector; they
// differ where several vector columns share a member (slod_lod_harmonic.hip).
constexpr int LOD_SLOTS = 8; // slots whose loads are in flight together in the PER_COL product

template <int S> // S = s, a constant here so that nothing stands between the loads
__device__ __forceinline__ double slod_lod_row_product_per_col(int p, int d, int cap, int NP, const double *__restrict__ values,
                                                               size_t ld_m, const uint32_t *__restrict__ cols,
                                                               const double *__restrict__ x, size_t ld, int col, int mcol)
{
  const size_t slot0 = (size_t)p * cap;
  double       acc = 0.0;
  for (int j0 = 0; j0 < cap; j0 += LOD_SLOTS)
    {
      bool   used[LOD_SLOTS];
      double a[LOD_SLOTS][S], xv[LOD_SLOTS][S];
#pragma unroll
      for (int u = 0; u < LOD_SLOTS; ++u)
        {
          // a slot past the end of the row reads the last one and adds nothing, like an unused slot
          const int      j = min(j0 + u, cap - 1);
          const uint32_t q = cols[slot0 + j];
          used[u]          = q < (uint32_t)NP && j0 + u < cap;
          const size_t qs = (size_t)(used[u] ? q : (uint32_t)p) * S, at = (slot0 + j) * S * S + d * S;
#pragma unroll
          for (int e = 0; e < S; ++e)
            {
              a[u][e]  = values[(at + e) * ld_m + mcol];
              xv[u][e] = x[(qs + e) * ld + col];
            }
        }
#pragma unroll
      for (int u = 0; u < LOD_SLOTS; ++u)
#pragma unroll
        for (int e = 0; e < S; ++e)
          {
            const double t = fma(a[u][e], xv[u][e], acc);
            acc            = used[u] ? t : acc;
          }
    }
  return acc;
}

template <bool PER_COL = false>
__device__ __forceinline__ double slod_lod_row_product(int i, int s, int cap, int NP, const double *__restrict__ values,
                                                       const uint32_t *__restrict__ cols, const double *__restrict__ x, size_t ld,
                                                       int col, size_t ld_m = 1)
{
  const int    p = i / s, d = i - p * s;
  const size_t slot0 = (size_t)p * cap;
  double       acc = 0.0;
  if constexpr (PER_COL)
    return s == 1 ? slod_lod_row_product_per_col<1>(p, d, cap, NP, values, ld_m, cols, x, ld, col, col)
                  : slod_lod_row_product_per_col<2>(p, d, cap, NP, values, ld_m, cols, x, ld, col, col);
  for (int j = 0; j < cap; ++j)
    {
      // an unused slot (0xffffffff; anything >= NP) reads the row's own patch and adds nothing:
      // no branch, so lanes of different rows stay together
      const uint32_t q = cols[slot0 + j];
      const bool     used = q < (uint32_t)NP;
      const size_t   qs = (size_t)(used ? q : (uint32_t)p) * s;
      const double  *a = values + (slot0 + j) * s * s + d * s;
      for (int e = 0; e < s; ++e)
        {
          const double t = fma(a[e], x[(qs + e) * ld + col], acc);
          acc            = used ? t : acc;
        }
    }
  return acc;
}

// buf[row][c] over the rows of a group, ascending
__device__ __forceinline__ double slod_lod_group_sum(const double (*buf)[LOD_COLS], int c)
{
  double s = buf[0][c];
#pragma unroll
  for (int i = 1; i < LOD_ROWS; ++i)
    s += buf[i][c];
  return s;
}

// partial[g][col] over the groups, ascending; ld: the columns of partial
__device__ __forceinline__ double slod_lod_ordered_sum(const double *partial, int ngroup, int ld, int col)
{
  double s = 0.0;
  for (int g = 0; g < ngroup; ++g)
    s += partial[(size_t)g * ld + col];
  return s;
}
#endif
