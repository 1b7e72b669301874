// The product of one block row with one column of a coarse multi-vector, shared by the CG of slod_lod_solve_multi
// (slod_lod_multi.hip), by slod_lod_apply_multi / slod_lod_theta_steps (slod_lod_time.hip) and by the bilinear form and
// the right-hand side of the Newmark stepper (slod_lod_wave.hip): one fma chain over the slots of the row in ascending
// order, so all give the same bits for the same matrix and column.
#ifndef SLOD_LOD_ROWS_HIP_H
#define SLOD_LOD_ROWS_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// sum_j sum_e values[(p cap + j) s s + d s + e] x[(cols[p cap + j] s + e) ld + col] for row i = p s + d
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
#endif
