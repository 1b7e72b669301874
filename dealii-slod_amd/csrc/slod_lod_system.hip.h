// The bodies of the three kernels of the global LOD system (A_LOD block rows, C^T f, C u_H), defined once for the
// single-problem kernels of slod_lod_system.hip and the ensemble kernels of slod_lod_ensemble.hip: the two differ in
// which slab, load and output a block works on and in the stride of its stores, never in an order of summation.
#ifndef SLOD_LOD_SYSTEM_HIP_H
#define SLOD_LOD_SYSTEM_HIP_H
#include "slod_host.h"
#include "slod_grid.hip.h"

namespace
{
  // ---------------------------------------------------------------------------------
  // A_LOD block row `row` = patch p.  Block of 256 threads, wave w = the candidate neighbours j = w, w+4, ...
  // (offsets of the centre cell in [-(2l+1), 2l+1]^2: patches further apart share no node).  Entry e of the row's
  // values goes to values[((row cap) s s + e) ld]; cols NULL: the columns are not written.
  // ---------------------------------------------------------------------------------
  __device__ __forceinline__ void lod_matrix_row(const SlodGrid &G, uint32_t p, size_t row, const double *basis,
                                                 const double *premult, size_t stride, double *values, size_t ld,
                                                 uint32_t *cols)
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = G.spacedim, n = G.n_sub, cap = grid_row_capacity(G);
    int       pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent  pe = grid_extent(G, pcx, pcy);
    const int     pnx = pe.mx * n + 1, pny = pe.my * n + 1, pnf = s * pnx * pny;
    const double *phi = basis + (size_t)p * stride;
    for (int j = wave; j < cap; j += 4)
      {
        const size_t   out = row * cap + j;
        const PairGeom pg = grid_pair(G, pcx, pcy, pe, j);
        const uint32_t q  = pg.q;
        const Extent   qe = pg.qe;
        const int      qnx = qe.mx * n + 1, qny = qe.my * n + 1, qnf = s * qnx * qny;
        const int      xa = pg.xa, ya = pg.ya, w = pg.w, hgt = pg.hgt;
        double    acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        if (w > 0 && hgt > 0)
          {
            const double *psi = premult + (size_t)q * stride;
            for (int idx = lane; idx < w * hgt; idx += 64)
              {
                const int iy = idx / w, ix = idx - iy * w;
                const int np = (xa + ix - pe.x0 * n) + (ya + iy - pe.y0 * n) * pnx;
                const int nq = (xa + ix - qe.x0 * n) + (ya + iy - qe.y0 * n) * qnx;
                for (int c = 0; c < s; ++c)
                  for (int d = 0; d < s; ++d)
                    {
                      const double ph = phi[(size_t)d * pnf + s * np + c];
                      for (int e = 0; e < s; ++e)
                        acc[d][e] = fma(ph, psi[(size_t)e * qnf + s * nq + c], acc[d][e]);
                    }
              }
          }
        for (int d = 0; d < s; ++d)
          for (int e = 0; e < s; ++e)
            {
              double v = acc[d][e];
              for (int off = 32; off > 0; off >>= 1)
                v += __shfl_xor(v, off, 64);
              if (lane == 0)
                values[(out * s * s + d * s + e) * ld] = v;
            }
        if (lane == 0 && cols)
          cols[out] = pg.col();
      }
  }

  // C^T f for block row `row` = patch p: block of 256 threads over all its nodes; out[(row s + d) ld]
  __device__ __forceinline__ void lod_rhs_row(const SlodGrid &G, uint32_t p, size_t row, const double *basis, size_t stride,
                                              const double *frhs, double *out, size_t ld)
  {
    __shared__ double red[4][2];
    const int         s = G.spacedim, n = G.n_sub, NEp = G.N * n + 1;
    int               pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent  pe = grid_extent(G, pcx, pcy);
    const int     pnx = pe.mx * n + 1, pny = pe.my * n + 1, pnf = s * pnx * pny;
    const double *phi = basis + (size_t)p * stride;
    double        acc[2] = {0.0, 0.0};
    for (int node = threadIdx.x; node < pnx * pny; node += 256)
      {
        const int iy = node / pnx, ix = node - iy * pnx;
        const int gn = (pe.x0 * n + ix) + (pe.y0 * n + iy) * NEp;
        for (int c = 0; c < s; ++c)
          {
            const double f = frhs[(size_t)gn * s + c];
            for (int d = 0; d < s; ++d)
              acc[d] = fma(phi[(size_t)d * pnf + s * node + c], f, acc[d]);
          }
      }
    for (int d = 0; d < s; ++d)
      {
        double v = acc[d];
        for (int off = 32; off > 0; off >>= 1)
          v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0)
          red[threadIdx.x >> 6][d] = v;
      }
    __syncthreads();
    if (threadIdx.x < s)
      out[(row * s + threadIdx.x) * ld] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  }

  // u_fine = C u_H at the global fine node gn (< (NE+1)^2): gather over the patches that contain it; u[(p s + d) ld]
  __device__ __forceinline__ void lod_reconstruct_node(const SlodGrid &G, int gn, const double *basis, size_t stride,
                                                       const double *u, size_t ld, double *fine)
  {
    const int s = G.spacedim, n = G.n_sub, NEp = G.N * n + 1, l = G.oversampling;
    const int X = gn % NEp, Y = gn / NEp;
    // cells whose closure contains the node, widened by the oversampling
    const int cxl = max((X + n - 1) / n - 1 - l, 0), cxh = min(X / n + l, G.N - 1);
    const int cyl = max((Y + n - 1) / n - 1 - l, 0), cyh = min(Y / n + l, G.N - 1);
    double    acc[2] = {0.0, 0.0};
    for (int cy = cyl; cy <= cyh; ++cy)
      for (int cx = cxl; cx <= cxh; ++cx)
        {
          const Extent e = grid_extent(G, cx, cy);
          const int    ix = X - e.x0 * n, iy = Y - e.y0 * n;
          if (ix < 0 || ix > e.mx * n || iy < 0 || iy > e.my * n)
            continue;
          const uint32_t p   = grid_pid(G, cx, cy);
          const int      pnx = e.mx * n + 1, pnf = s * pnx * (e.my * n + 1);
          const double  *phi = basis + (size_t)p * stride;
          for (int d = 0; d < s; ++d)
            {
              const double ud = u[((size_t)p * s + d) * ld];
              for (int c = 0; c < s; ++c)
                acc[c] = fma(phi[(size_t)d * pnf + s * (ix + iy * pnx) + c], ud, acc[c]);
            }
        }
    for (int c = 0; c < s; ++c)
      fine[(size_t)gn * s + c] = acc[c];
  }
} // namespace
#endif
