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
  // Slot j of the block row of a patch p is the candidate neighbour q whose centre cell lies at offset
  // (j % span, j / span) - span / 2 from p's, span = 4 l + 3 (patches further apart share no node); a row has span^2
  // slots.  The overlap of the two closed patches is w x hgt global fine nodes from (xa, ya): a pair that shares only a
  // line of nodes has w or hgt = 1, a pair that shares none has one <= 0, a centre outside the domain gives w = hgt = 0.
  __host__ __device__ inline int grid_row_capacity(const SlodGrid &G) { return (4 * G.oversampling + 3) * (4 * G.oversampling + 3); }
  struct PairGeom
  {
    uint32_t q;
    Extent   qe;
    int      xa, ya, w, hgt;
    // the column the slot holds in the pattern of A_LOD and M_LOD: q when the patches share a node
    __host__ __device__ uint32_t col() const { return w > 0 && hgt > 0 ? q : 0xffffffffu; }
  };
  __host__ __device__ inline PairGeom grid_pair(const SlodGrid &G, int pcx, int pcy, const Extent &pe, int j)
  {
    PairGeom  g{};
    const int n = G.n_sub, span = 4 * G.oversampling + 3;
    const int qcx = pcx + j % span - (span / 2), qcy = pcy + j / span - (span / 2);
    if (qcx < 0 || qcx >= G.N || qcy < 0 || qcy >= G.N)
      return g;
    g.q  = grid_pid(G, qcx, qcy);
    g.qe = grid_extent(G, qcx, qcy);
    // overlap in global fine-node coordinates (inclusive)
    const Extent &qe = g.qe;
    const int     xb = min(pe.x0 + pe.mx, qe.x0 + qe.mx) * n, yb = min(pe.y0 + pe.my, qe.y0 + qe.my) * n;
    g.xa  = max(pe.x0, qe.x0) * n;
    g.ya  = max(pe.y0, qe.y0) * n;
    g.w   = xb - g.xa + 1;
    g.hgt = yb - g.ya + 1;
    return g;
  }
  // descriptor -> public patch layout (slod_plan_patch_layout, slod_device_patch_layout), everything from the
  // descriptor the device built -- except the position of a full patch under the reuse quirk Q1: there
  // k_make_desc stores the first full patch's coefficient origin in (ox, oy), and the patch's own origin is
  // recomputed from its id.
  inline void slod_desc_to_info(const slod_handle *h, uint32_t pid, const SlodPatchDesc &d, slod_patch_info *info)
  {
    const int n = h->cfg.n_subdivisions, s = h->cfg.spacedim, full = 2 * h->cfg.oversampling + 1;
    *info       = slod_patch_info();
    info->x0    = d.ox / n;
    info->y0    = d.oy / n;
    if (h->cfg.constant_coefficients && h->first_full >= 0 && d.mx == full && d.my == full)
      {
        const SlodGrid G = slod_grid_of(h);
        int            cx, cy;
        grid_centre(G, pid, cx, cy);
        const Extent e = grid_extent(G, cx, cy);
        info->x0       = e.x0;
        info->y0       = e.y0;
      }
    info->cx = info->x0 + d.ccx;
    info->cy = info->y0 + d.ccy;
    info->mx = d.mx;
    info->my = d.my;
    info->nx = d.nx;
    info->ny = d.ny;
    for (int k = 0; k < 4; ++k)
      info->side_domain[k] = (d.flags >> k) & 1;
    info->n_fine     = s * (d.nx + 1) * (d.ny + 1);
    info->n_internal = s * (d.nx - 1) * (d.ny - 1);
    info->n_boundary = d.n_b;
    info->n_coarse   = d.n_c;
    info->is_lod     = (d.flags & SLOD_F_LOD) ? 1 : 0;
  }
} // namespace
#endif
