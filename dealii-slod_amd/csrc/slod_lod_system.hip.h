// The bodies of the three kernels of the global LOD system (A_LOD block rows, C^T f, C u_H), defined once for the
// single-problem kernels of slod_lod_system.hip and the ensemble kernels of slod_lod_ensemble.hip: the two differ in
// which slab, load and output a block works on and in the stride of its stores, never in an order of summation.
// The entries of A_LOD and M_LOD are per-slot bodies: the full-row kernels and the in-place update after a local
// coefficient change (slod_lod_update.hip) call the same one.
#ifndef SLOD_LOD_SYSTEM_HIP_H
#define SLOD_LOD_SYSTEM_HIP_H
#include "slod_host.h"
#include "slod_grid.hip.h"

namespace
{
  // ---------------------------------------------------------------------------------
  // One entry of A_LOD: slot `out` = (row, j) of the block row of patch p (extent pe, vectors phi), pair geometry pg
  // of the slot, computed by ONE wave in a fixed order (lanes over the nodes of the overlap rectangle, then the
  // butterfly), so that an entry recomputed alone (slod_lod_update.hip) has the bits of the full row.  Entry e of the
  // slot goes to values[(out s s + e) ld].
  // ---------------------------------------------------------------------------------
  __device__ __forceinline__ void lod_matrix_slot(const SlodGrid &G, const Extent &pe, const double *phi, const PairGeom &pg,
                                                  const double *premult, size_t stride, size_t out, double *values, size_t ld)
  {
    const int      lane = threadIdx.x & 63;
    const int      s = G.spacedim, n = G.n_sub;
    const int      pnx = pe.mx * n + 1, pny = pe.my * n + 1, pnf = s * pnx * pny;
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
  }

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
    const int cap = grid_row_capacity(G);
    int       pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent  pe = grid_extent(G, pcx, pcy);
    const double *phi = basis + (size_t)p * stride;
    for (int j = wave; j < cap; j += 4)
      {
        const size_t   out = row * cap + j;
        const PairGeom pg = grid_pair(G, pcx, pcy, pe, j);
        lod_matrix_slot(G, pe, phi, pg, premult, stride, out, values, ld);
        if (lane == 0 && cols)
          cols[out] = pg.col();
      }
  }

  // ---------------------------------------------------------------------------------
  // One entry of M_LOD, the counterpart of lod_matrix_slot for k_lod_mass (slod_lod_time.hip): lanes = the fine
  // elements of the intersection rectangle of the two closed patches (phi vanishes on every patch rim, so these
  // elements carry the whole integral).  Lanes run along ix: the corner loads of neighbouring lanes are neighbouring
  // doubles (spacedim 1) or neighbouring pairs (spacedim 2).
  //
  // Element form, Q1 consistent mass rho h^2/36 [[4,2,2,1],[2,4,1,2],[2,1,4,2],[1,2,2,4]] = rho h^2/36 (J+I)x(J+I):
  //   p^T (J+I)x(J+I) q = (sum p)(sum q) + sum_rows (row sum p)(row sum q) + sum_cols (col sum p)(col sum q) + p.q
  // Every product pairs a quantity of p with the same quantity of q and nothing is contracted into an fma, so the
  // form is symmetric in (p, q) bit for bit; with the same lanes, the same component order and the same wave
  // reduction on both sides, M[(p,d),(q,e)] and M[(q,e),(p,d)] are the same bits.  Entry e of the slot goes to
  // values[(out S S + e) ld].
  // ---------------------------------------------------------------------------------
  template <int S>
  __device__ __forceinline__ void lod_mass_slot(const SlodGrid &G, const Extent &pe, const double *phi, const PairGeom &pg,
                                                const double *basis, size_t stride, const double *rho, double scale, size_t out,
                                                double *values, size_t ld)
  {
#pragma clang fp contract(off)
    const int      lane = threadIdx.x & 63;
    const int      n = G.n_sub, NE = G.N * n;
    const int      pnx = pe.mx * n + 1, pny = pe.my * n + 1, pnf = S * pnx * pny;
    // the overlap is w x hgt nodes, (w - 1) x (hgt - 1) elements
    const uint32_t q  = pg.q;
    const Extent   qe = pg.qe;
    const int      qnx = qe.mx * n + 1, qny = qe.my * n + 1, qnf = S * qnx * qny;
    const int      xa = pg.xa, ya = pg.ya, w = pg.w, hgt = pg.hgt;
    double    acc[S][S];
#pragma unroll
    for (int d = 0; d < S; ++d)
#pragma unroll
      for (int e = 0; e < S; ++e)
        acc[d][e] = 0.0;
    if (w > 1 && hgt > 1)
      {
        const double *phq = basis + (size_t)q * stride;
        const int     we = w - 1;
        for (int idx = lane; idx < we * (hgt - 1); idx += 64)
          {
            const int    iy = idx / we, ix = idx - iy * we;
            const int    np = (xa + ix - pe.x0 * n) + (ya + iy - pe.y0 * n) * pnx;
            const int    nq = (xa + ix - qe.x0 * n) + (ya + iy - qe.y0 * n) * qnx;
            const double r  = rho ? rho[(size_t)(ya + iy) * NE + (xa + ix)] : 1.0;
#pragma unroll
            for (int c = 0; c < S; ++c)
              {
                // corner values and their sums, [d] of the row patch, [e] of the column patch
                double a[S][4], b[S][4];
#pragma unroll
                for (int d = 0; d < S; ++d)
                  {
                    const double *v = phi + (size_t)d * pnf + c;
                    a[d][0]         = v[S * np];
                    a[d][1]         = v[S * (np + 1)];
                    a[d][2]         = v[S * (np + pnx)];
                    a[d][3]         = v[S * (np + pnx + 1)];
                    const double *u = phq + (size_t)d * qnf + c;
                    b[d][0]         = u[S * nq];
                    b[d][1]         = u[S * (nq + 1)];
                    b[d][2]         = u[S * (nq + qnx)];
                    b[d][3]         = u[S * (nq + qnx + 1)];
                  }
#pragma unroll
                for (int d = 0; d < S; ++d)
#pragma unroll
                  for (int e = 0; e < S; ++e)
                    {
                      const double ar0 = a[d][0] + a[d][1], ar1 = a[d][2] + a[d][3];
                      const double ac0 = a[d][0] + a[d][2], ac1 = a[d][1] + a[d][3];
                      const double br0 = b[e][0] + b[e][1], br1 = b[e][2] + b[e][3];
                      const double bc0 = b[e][0] + b[e][2], bc1 = b[e][1] + b[e][3];
                      const double all = (ar0 + ar1) * (br0 + br1);
                      const double row = ar0 * br0 + ar1 * br1;
                      const double col = ac0 * bc0 + ac1 * bc1;
                      const double dot = (a[d][0] * b[e][0] + a[d][1] * b[e][1]) + (a[d][2] * b[e][2] + a[d][3] * b[e][3]);
                      acc[d][e]        = acc[d][e] + r * ((all + dot) + (row + col));
                    }
              }
          }
      }
#pragma unroll
    for (int d = 0; d < S; ++d)
#pragma unroll
      for (int e = 0; e < S; ++e)
        {
          double v = acc[d][e];
          for (int off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off, 64);
          if (lane == 0)
            values[(out * S * S + d * S + e) * ld] = v * scale;
        }
  }

  // M_LOD block row `row` = patch p, the counterpart of lod_matrix_row: wave w = the candidate neighbours j = w, w+4, ...
  // The pattern is that of lod_matrix_row: a pair that shares only a line of nodes keeps its column, value 0.
  template <int S>
  __device__ __forceinline__ void lod_mass_row(const SlodGrid &G, uint32_t p, size_t row, const double *basis, size_t stride,
                                               const double *rho, double scale, double *values, size_t ld, uint32_t *cols)
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap = grid_row_capacity(G);
    int       pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent  pe = grid_extent(G, pcx, pcy);
    const double *phi = basis + (size_t)p * stride;
    for (int j = wave; j < cap; j += 4)
      {
        const size_t   out = row * cap + j;
        const PairGeom pg = grid_pair(G, pcx, pcy, pe, j);
        lod_mass_slot<S>(G, pe, phi, pg, basis, stride, rho, scale, out, values, ld);
        if (lane == 0 && cols)
          cols[out] = pg.col();
      }
  }

  // Word w = ((p cap + j) s + d) s + e of (A + A^T) / 2 on a full set of block rows whose words are ld apart: the partner
  // is A[q,j'][e][d], q = cols[p,j], j' the slot of p in row q (0 when there is none).  One rounding of the sum, an exact
  // halving, both commutative: the result is symmetric bit for bit.
  __device__ __forceinline__ double lod_symmetrize_word(int NP, int s, int cap, const double *values, size_t ld, const uint32_t *cols,
                                                        size_t w)
  {
#pragma clang fp contract(off)
    const size_t   ss = (size_t)s * s, slot = w / ss;
    const int      de = (int)(w - slot * ss), d = de / s, e = de - d * s;
    const uint32_t p = (uint32_t)(slot / cap), q = cols[slot];
    if (q >= (uint32_t)NP)
      return 0.0;
    double t = 0.0;
    for (int j = 0; j < cap; ++j)
      if (cols[(size_t)q * cap + j] == p)
        {
          t = values[(((size_t)q * cap + j) * ss + e * s + d) * ld];
          break;
        }
    return 0.5 * (values[w * ld] + t);
  }

  // alpha a + beta b, two roundings of the products and one of the sum (no fma)
  __device__ __forceinline__ double lod_combine_word(double alpha, double a, double beta, double b)
  {
#pragma clang fp contract(off)
    const double ta = alpha * a, tb = beta * b;
    return ta + tb;
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
