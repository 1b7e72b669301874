// The global LOD system, the consumer of the per-patch basis construction:
// A_LOD = C^T (A C),  C^T f,  its solve and the fine-scale reconstruction (reference assemble_global_matrix
// LOD.cc:860-973, solve :976-1002, :1251), for one load vector and for n_rhs at once.
// Everything is index arithmetic on the patch-lexicographic layout of include/slod.h: the overlap of
// two patches is a rectangle of global fine nodes.  These kernels are HBM/L2-bound gathers and
// reductions (no MFMA shape in them); one wave per patch pair keeps every reduction inside a wave.
#include "slod_host.h"
#include "slod_cg.hip.h"
#include "slod_lod_system.hip.h"

#include <algorithm>
#include <vector>

namespace
{
  // The three kernels of one problem; their bodies are slod_lod_system.hip.h.  Block = one row patch.
  __global__ __launch_bounds__(256) void k_lod_matrix(const SlodGrid G, const uint32_t *rows, const double *basis,
                                                     const double *premult, size_t stride, double *values,
                                                     uint32_t *cols)
  {
    lod_matrix_row(G, rows[blockIdx.x], blockIdx.x, basis, premult, stride, values, 1, cols);
  }

  __global__ __launch_bounds__(256) void k_lod_rhs(const SlodGrid G, const uint32_t *rows, const double *basis,
                                                  size_t stride, const double *frhs, double *out)
  {
    lod_rhs_row(G, rows[blockIdx.x], blockIdx.x, basis, stride, frhs, out, 1);
  }

  // one thread per global fine node
  __global__ __launch_bounds__(256) void k_lod_reconstruct(const SlodGrid G, const double *basis, size_t stride,
                                                          const double *u, double *fine)
  {
    const int NEp = G.N * G.n_sub + 1, gn = blockIdx.x * 256 + threadIdx.x;
    if (gn < NEp * NEp)
      lod_reconstruct_node(G, gn, basis, stride, u, 1, fine);
  }

  // ---- the same two products for n_rhs load vectors at once (slod_lod_rhs_multi, slod_lod_reconstruct_multi).
  // Fine multi-vectors are field-major (column c at + c * ld_fine), coarse ones interleaved ([row][column]).
  // A block takes a tile of MULTI_TILE columns (blockIdx.y): a phi value is loaded once and used for every
  // column of the tile.
  constexpr int MULTI_TILE = 16;
  // C^T F: block = one patch x one column tile, threads = the patch's nodes (reads of F coalesced per column)
  template <int S>
  __global__ __launch_bounds__(256) void k_lod_rhs_multi(const SlodGrid G, const uint32_t *rows, const double *basis,
                                                        size_t stride, const double *frhs, size_t ld_fine, int n_rhs,
                                                        double *out, size_t ld_out)
  {
    __shared__ double red[4][S * MULTI_TILE];
    const int         n = G.n_sub, NEp = G.N * n + 1;
    const uint32_t    p = rows[blockIdx.x];
    const int         c0 = blockIdx.y * MULTI_TILE, nc = min(MULTI_TILE, n_rhs - c0);
    int               pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent  pe = grid_extent(G, pcx, pcy);
    const int     pnx = pe.mx * n + 1, pny = pe.my * n + 1, pnf = S * pnx * pny;
    const double *phi = basis + (size_t)p * stride;
    double        acc[S][MULTI_TILE];
#pragma unroll
    for (int d = 0; d < S; ++d)
#pragma unroll
      for (int k = 0; k < MULTI_TILE; ++k)
        acc[d][k] = 0.0;
    for (int node = threadIdx.x; node < pnx * pny; node += 256)
      {
        const int iy = node / pnx, ix = node - iy * pnx;
        const int gn = (pe.x0 * n + ix) + (pe.y0 * n + iy) * NEp;
        double    ph[S][S]; // [d][c]
#pragma unroll
        for (int d = 0; d < S; ++d)
#pragma unroll
          for (int c = 0; c < S; ++c)
            ph[d][c] = phi[(size_t)d * pnf + S * node + c];
#pragma unroll
        for (int k = 0; k < MULTI_TILE; ++k)
          if (k < nc)
            {
              const double *f = frhs + (size_t)(c0 + k) * ld_fine + (size_t)gn * S;
#pragma unroll
              for (int c = 0; c < S; ++c)
                {
                  const double fc = f[c];
#pragma unroll
                  for (int d = 0; d < S; ++d)
                    acc[d][k] = fma(ph[d][c], fc, acc[d][k]);
                }
            }
      }
#pragma unroll
    for (int d = 0; d < S; ++d)
#pragma unroll
      for (int k = 0; k < MULTI_TILE; ++k)
        {
          double v = acc[d][k];
          for (int off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off, 64);
          if ((threadIdx.x & 63) == 0)
            red[threadIdx.x >> 6][d * MULTI_TILE + k] = v;
        }
    __syncthreads();
    if ((int)threadIdx.x < S * MULTI_TILE)
      {
        const int d = threadIdx.x / MULTI_TILE, k = threadIdx.x - d * MULTI_TILE;
        if (k < nc)
          out[((size_t)blockIdx.x * S + d) * ld_out + c0 + k] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
      }
  }

  // U_fine = C U_H: one thread per global fine node and column tile; the loop over the covering patches and
  // the order of the fma chain are those of k_lod_reconstruct, so every field equals the single-vector result
  template <int S>
  __global__ __launch_bounds__(256) void k_lod_reconstruct_multi(const SlodGrid G, const double *basis, size_t stride,
                                                                const double *u, size_t ld_u, int n_rhs, double *fine,
                                                                size_t ld_fine)
  {
    const int n = G.n_sub, NEp = G.N * n + 1, l = G.oversampling;
    const int gn = blockIdx.x * 256 + threadIdx.x;
    const int c0 = blockIdx.y * MULTI_TILE, nc = min(MULTI_TILE, n_rhs - c0);
    if (gn >= NEp * NEp)
      return;
    const int X = gn % NEp, Y = gn / NEp;
    const int cxl = max((X + n - 1) / n - 1 - l, 0), cxh = min(X / n + l, G.N - 1);
    const int cyl = max((Y + n - 1) / n - 1 - l, 0), cyh = min(Y / n + l, G.N - 1);
    double    acc[MULTI_TILE][S];
#pragma unroll
    for (int k = 0; k < MULTI_TILE; ++k)
#pragma unroll
      for (int c = 0; c < S; ++c)
        acc[k][c] = 0.0;
    for (int cy = cyl; cy <= cyh; ++cy)
      for (int cx = cxl; cx <= cxh; ++cx)
        {
          const Extent e = grid_extent(G, cx, cy);
          const int    ix = X - e.x0 * n, iy = Y - e.y0 * n;
          if (ix < 0 || ix > e.mx * n || iy < 0 || iy > e.my * n)
            continue;
          const uint32_t p   = grid_pid(G, cx, cy);
          const int      pnx = e.mx * n + 1, pnf = S * pnx * (e.my * n + 1);
          const double  *phi = basis + (size_t)p * stride;
#pragma unroll
          for (int d = 0; d < S; ++d)
            {
              double ph[S];
#pragma unroll
              for (int c = 0; c < S; ++c)
                ph[c] = phi[(size_t)d * pnf + S * (ix + iy * pnx) + c];
              const double *ud = u + ((size_t)p * S + d) * ld_u + c0; // contiguous in the column
#pragma unroll
              for (int k = 0; k < MULTI_TILE; ++k)
                if (k < nc)
                  {
                    const double uk = ud[k];
#pragma unroll
                    for (int c = 0; c < S; ++c)
                      acc[k][c] = fma(ph[c], uk, acc[k][c]);
                  }
            }
        }
#pragma unroll
    for (int k = 0; k < MULTI_TILE; ++k)
      if (k < nc)
#pragma unroll
        for (int c = 0; c < S; ++c)
          fine[(size_t)(c0 + k) * ld_fine + (size_t)gn * S + c] = acc[k][c];
  }

  // ---- Jacobi-preconditioned CG on the block rows (device scalars: no host round trip per step): the product
  // and the init kernel of slod_lod_solve; the rest of the recurrence and its driver are slod_cg.hip.h
  __global__ void k_cg_spmv_dot(int nrow, int s, int cap, const double *values, const uint32_t *cols, const double *x,
                                double *y, CgScalars *sc)
  {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double    part = 0.0;
    if (i < nrow)
      {
        const int p = i / s, d = i - p * s;
        double    acc = 0.0;
        for (int j = 0; j < cap; ++j)
          {
            const uint32_t q = cols[(size_t)p * cap + j];
            if (q == 0xffffffffu)
              continue;
            for (int e = 0; e < s; ++e)
              acc = fma(values[((size_t)p * cap + j) * s * s + d * s + e], x[(size_t)q * s + e], acc);
          }
        y[i] = acc;
        part = acc * x[i];
      }
    for (int off = 32; off > 0; off >>= 1)
      part += __shfl_xor(part, off, 64);
    if ((threadIdx.x & 63) == 0 && part != 0.0)
      atomicAdd(&sc->pAp, part);
  }
  __global__ void k_cg_init(int nrow, int s, int cap, const double *values, const uint32_t *cols, const double *rhs,
                            double *x, double *r, double *z, double *pv, double *dinv, CgScalars *sc)
  {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double    a = 0.0, b = 0.0;
    if (i < nrow)
      {
        const int p = i / s, d = i - p * s;
        double    diag = 1.0;
        for (int j = 0; j < cap; ++j)
          if (cols[(size_t)p * cap + j] == (uint32_t)p)
            diag = values[((size_t)p * cap + j) * s * s + d * s + d];
        dinv[i] = diag != 0.0 ? 1.0 / diag : 1.0;
        x[i]    = 0.0;
        r[i]    = rhs[i];
        z[i]    = dinv[i] * rhs[i];
        pv[i]   = z[i];
        a       = r[i] * z[i];
        b       = r[i] * r[i];
      }
    for (int off = 32; off > 0; off >>= 1)
      {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
      }
    if ((threadIdx.x & 63) == 0)
      {
        atomicAdd(&sc->rz, a);
        atomicAdd(&sc->rhs2, b);
        atomicAdd(&sc->rr, b);
      }
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_row_capacity(const slod_handle *h)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  return grid_row_capacity(slod_grid_of(h));
}

int slod_lod_pattern(const slod_handle *h, uint32_t patch_id, uint32_t *neighbours, size_t capacity)
{
  if (!h || !neighbours)
    return SLOD_ERR_ARGUMENT;
  if (patch_id >= (uint32_t)h->NP)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_pattern: patch id out of range");
  const SlodGrid G = slod_grid_of(h);
  int            cx, cy;
  grid_centre(G, patch_id, cx, cy);
  const Extent          pe = grid_extent(G, cx, cy);
  std::vector<uint32_t> nb;
  for (int j = 0; j < grid_row_capacity(G); ++j)
    {
      const uint32_t q = grid_pair(G, cx, cy, pe, j).col();
      if (q != 0xffffffffu)
        nb.push_back(q);
    }
  std::sort(nb.begin(), nb.end());
  if (capacity < nb.size())
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_pattern: buffer too small");
  std::copy(nb.begin(), nb.end(), neighbours);
  return (int)nb.size();
}

int slod_lod_matrix(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, const double *d_premult,
                    size_t stride, double *d_values, uint32_t *d_cols, void *hip_stream)
{
  if (!h || (n_rows && (!rows || !d_basis || !d_premult || !d_values || !d_cols)))
    return SLOD_ERR_ARGUMENT;
  if (n_rows == 0)
    return SLOD_OK;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  SlodDevBuf<uint32_t> d_rows;
  if (const int rc = slod_upload_rows(h, nullptr, rows, n_rows, st, &d_rows))
    return rc;
  hipLaunchKernelGGL(k_lod_matrix, dim3((unsigned)n_rows), dim3(256), 0, st, slod_grid_of(h), d_rows.get(), d_basis, d_premult,
                     stride, d_values, d_cols);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); // d_rows is freed on return
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_matrix");
}

int slod_lod_rhs(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, size_t stride,
                 const double *d_fine_rhs, double *d_out, void *hip_stream)
{
  if (!h || (n_rows && (!rows || !d_basis || !d_fine_rhs || !d_out)))
    return SLOD_ERR_ARGUMENT;
  if (n_rows == 0)
    return SLOD_OK;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  SlodDevBuf<uint32_t> d_rows;
  if (const int rc = slod_upload_rows(h, nullptr, rows, n_rows, st, &d_rows))
    return rc;
  hipLaunchKernelGGL(k_lod_rhs, dim3((unsigned)n_rows), dim3(256), 0, st, slod_grid_of(h), d_rows.get(), d_basis, stride,
                     d_fine_rhs, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); // d_rows is freed on return
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_rhs");
}

int slod_lod_solve(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_rhs, double *d_u,
                   double rel_tol, int max_iterations, double *rel_residual)
{
  if (!h || !d_values || !d_cols || !d_rhs || !d_u || max_iterations < 0)
    return SLOD_ERR_ARGUMENT;
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const int             s = h->cfg.spacedim, cap = slod_lod_row_capacity(h), nrow = h->NP * s;
  const int             nblk = (nrow + 255) / 256;
  SlodDevBuf<double>    work;
  SlodDevBuf<CgScalars> sc;
  hipError_t            e = work.alloc((size_t)5 * nrow);
  if (e == hipSuccess)
    e = sc.alloc(1);
  if (e == hipSuccess)
    e = hipMemsetAsync(sc.get(), 0, sizeof(CgScalars), st);
  int it = 0;
  if (e == hipSuccess)
    {
      double *r = work.get(), *z = r + nrow, *pv = r + 2 * (size_t)nrow, *Ap = r + 3 * (size_t)nrow, *dinv = r + 4 * (size_t)nrow;
      hipLaunchKernelGGL(k_cg_init, dim3(nblk), dim3(256), 0, st, nrow, s, cap, d_values, d_cols, d_rhs, d_u, r, z, pv, dinv,
                         sc.get());
      // the driver synchronises st before it returns: work and sc are idle when they are freed
      const auto step = [&] {
        hipLaunchKernelGGL(k_cg_spmv_dot, dim3(nblk), dim3(256), 0, st, nrow, s, cap, d_values, d_cols, pv, Ap, sc.get());
        hipLaunchKernelGGL(k_cg_update_xr, dim3(nblk), dim3(256), 0, st, nrow, pv, Ap, dinv, d_u, r, z, sc.get());
        hipLaunchKernelGGL(k_cg_update_p, dim3(nblk), dim3(256), 0, st, nrow, z, pv, sc.get());
      };
      e = slod_cg_drive(st, sc.get(), 8, max_iterations, rel_tol, step, &it, rel_residual);
    }
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_lod_solve");
  return it;
}

int slod_lod_reconstruct(slod_handle *h, const double *d_basis, size_t stride, const double *d_u, double *d_fine,
                         void *hip_stream)
{
  if (!h || !d_basis || !d_u || !d_fine)
    return SLOD_ERR_ARGUMENT;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int NEp = h->NE + 1;
  hipLaunchKernelGGL(k_lod_reconstruct, dim3((unsigned)((NEp * NEp + 255) / 256)), dim3(256), 0, st, slod_grid_of(h),
                     d_basis, stride, d_u, d_fine);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_reconstruct");
}

int slod_lod_rhs_multi(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, size_t stride,
                       const double *d_fine_rhs, size_t ld_fine, int n_rhs, double *d_out, size_t ld_out, void *hip_stream)
{
  if (!h || (n_rows && (!rows || !d_basis || !d_fine_rhs || !d_out)))
    return SLOD_ERR_ARGUMENT;
  if (n_rhs < 1 || ld_out < (size_t)n_rhs)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_rhs_multi: n_rhs < 1 or ld_out < n_rhs");
  if (ld_fine < (size_t)(h->NE + 1) * (h->NE + 1) * h->cfg.spacedim)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_rhs_multi: ld_fine shorter than a fine field");
  if (n_rows == 0)
    return SLOD_OK;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  SlodDevBuf<uint32_t> d_rows;
  if (const int rc = slod_upload_rows(h, nullptr, rows, n_rows, st, &d_rows))
    return rc;
  const dim3 grid((unsigned)n_rows, (unsigned)((n_rhs + MULTI_TILE - 1) / MULTI_TILE));
  if (h->cfg.spacedim == 1)
    hipLaunchKernelGGL(k_lod_rhs_multi<1>, grid, dim3(256), 0, st, slod_grid_of(h), d_rows.get(), d_basis, stride, d_fine_rhs,
                       ld_fine, n_rhs, d_out, ld_out);
  else
    hipLaunchKernelGGL(k_lod_rhs_multi<2>, grid, dim3(256), 0, st, slod_grid_of(h), d_rows.get(), d_basis, stride, d_fine_rhs,
                       ld_fine, n_rhs, d_out, ld_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); // d_rows is freed on return
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_rhs_multi");
}

int slod_lod_reconstruct_multi(slod_handle *h, const double *d_basis, size_t stride, const double *d_u, size_t ld_u, int n_rhs,
                               double *d_fine, size_t ld_fine, void *hip_stream)
{
  if (!h || !d_basis || !d_u || !d_fine)
    return SLOD_ERR_ARGUMENT;
  if (n_rhs < 1 || ld_u < (size_t)n_rhs)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_reconstruct_multi: n_rhs < 1 or ld_u < n_rhs");
  if (ld_fine < (size_t)(h->NE + 1) * (h->NE + 1) * h->cfg.spacedim)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_reconstruct_multi: ld_fine shorter than a fine field");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int  NEp = h->NE + 1;
  const dim3 grid((unsigned)((NEp * NEp + 255) / 256), (unsigned)((n_rhs + MULTI_TILE - 1) / MULTI_TILE));
  if (h->cfg.spacedim == 1)
    hipLaunchKernelGGL(k_lod_reconstruct_multi<1>, grid, dim3(256), 0, st, slod_grid_of(h), d_basis, stride, d_u, ld_u, n_rhs,
                       d_fine, ld_fine);
  else
    hipLaunchKernelGGL(k_lod_reconstruct_multi<2>, grid, dim3(256), 0, st, slod_grid_of(h), d_basis, stride, d_u, ld_u, n_rhs,
                       d_fine, ld_fine);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_reconstruct_multi");
}

} // extern "C"
#pragma GCC visibility pop
