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
// over the slots of the row in ascending order
__device__ __forceinline__ double slod_lod_row_product(int i, int s, int cap, int NP, const double *__restrict__ values,
                                                       const uint32_t *__restrict__ cols, const double *__restrict__ x, size_t ld,
                                                       int col)
{
  const int    p = i / s, d = i - p * s;
  const size_t slot0 = (size_t)p * cap;
  double       acc = 0.0;
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
