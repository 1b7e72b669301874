// Index calculus on the coarse grid shared by host and device code of the global steps (slod_lod_system.hip,
// slod_plan_build.hip, slod_lod_time.hip): patch id <-> centre cell, and the extent of a patch in coarse cells.  The overlap of two
// patches is a rectangle of global fine nodes; everything derives from the scalars of SlodGrid (slod_host.h).
#ifndef SLOD_GRID_HIP_H
#define SLOD_GRID_HIP_H
#include "slod_host.h"

namespace
{
  // ---- index calculus shared by host and device (mirrors patch_geom() of slod_api.cpp) ----
  __host__ __device__ inline void grid_centre(const SlodGrid &G, uint32_t pid, int &cx, int &cy)
  {
    if (G.morton_bits < 0)
      {
        cx = (int)(pid % (uint32_t)G.N);
        cy = (int)(pid / (uint32_t)G.N);
        return;
      }
    cx = cy = 0;
    for (int b = 0; b < G.morton_bits; ++b)
      {
        cx |= (int)((pid >> (2 * b)) & 1u) << b;
        cy |= (int)((pid >> (2 * b + 1)) & 1u) << b;
      }
  }
  __host__ __device__ inline uint32_t grid_pid(const SlodGrid &G, int cx, int cy)
  {
    if (G.morton_bits < 0)
      return (uint32_t)(cx + G.N * cy);
    uint32_t p = 0;
    for (int b = 0; b < G.morton_bits; ++b)
      p |= ((uint32_t)((cx >> b) & 1) << (2 * b)) | ((uint32_t)((cy >> b) & 1) << (2 * b + 1));
    return p;
  }
  struct Extent
  {
    int x0, y0, mx, my; // coarse cells
  };
  __host__ __device__ inline Extent grid_extent(const SlodGrid &G, int cx, int cy)
  {
    Extent    e;
    const int l = G.oversampling;
    e.x0        = cx - l > 0 ? cx - l : 0;
    e.y0        = cy - l > 0 ? cy - l : 0;
    const int x1 = cx + l < G.N - 1 ? cx + l : G.N - 1, y1 = cy + l < G.N - 1 ? cy + l : G.N - 1;
    e.mx         = x1 - e.x0 + 1;
    e.my         = y1 - e.y0 + 1;
    return e;
  }
} // namespace
#endif
