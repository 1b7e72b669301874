// slod_lod_solve_multi: A_LOD U = F for n_rhs load vectors at once (the reference solves one, LOD.cc:976-1002).
// Every column runs the Jacobi-preconditioned CG recurrence of slod_lod_solve with scalars of its own; the
// columns share the reads of the block rows and the launches, nothing else.
//
// Tiling and summation order are those of slod_lod_tile.hip.h: a dot product is one partial per (group, column),
// and whoever needs the scalar sums the partials in ascending group order (every block for itself: no atomics, no
// fourth launch).  An iteration is three launches for all columns:
//   k_mcg_spmv       Y = A P, partials of p.Ap
//   k_mcg_update_xr  alpha = r.z / p.Ap;  x += alpha p, r -= alpha Ap, z = D^-1 r; partials of r.z and r.r
//   k_mcg_update_p   beta = r.z_new / r.z;  p = z + beta p
// The r.z partials are double-buffered by iteration parity, which replaces k_cg_rotate.  Every 8 iterations
// k_mcg_check sums the r.r partials and freezes the columns that have converged (their u is not written
// again); the host reads the flags back.
//
// PER_COL (slod_lod_solve_ensemble): column k reads a matrix of its own on the shared pattern, entry e at
// values[e ld_m + k], and a D^-1 of its own.  The kernels that touch the matrix or D^-1 carry the parameter; the
// recurrence, the tiling and every summation order are the same code.
#include "slod_lod_tile.hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace
{
  constexpr int SOLVE_MAX_BLOCKS = 256; // blocks per chunk

  struct McgVectors
  {
    double *r, *z, *p, *Ap; // [nrow][n_rhs]
    double *dinv;           // [nrow], PER_COL: [nrow][n_rhs]
    double *pAp, *rz[2], *rr; // partials [ngroup][n_rhs]
    double *rhs2, *rr_last; // [n_rhs]
    int    *active;         // [n_rhs]
  };

  template <bool PER_COL>
  __global__ void k_mcg_diag(int nrow, int s, int cap, int n_rhs, const double *values, size_t ld_m, const uint32_t *cols,
                             double *dinv)
  {
    const size_t w = (size_t)blockIdx.x * LOD_BLOCK + threadIdx.x; // PER_COL: (row, column), else the row
    if (w >= (PER_COL ? (size_t)nrow * n_rhs : (size_t)nrow))
      return;
    const int i = PER_COL ? (int)(w / n_rhs) : (int)w, col = PER_COL ? (int)(w - (size_t)i * n_rhs) : 0;
    const int p = i / s, d = i - p * s;
    double    diag = 1.0;
    for (int j = 0; j < cap; ++j)
      if (cols[(size_t)p * cap + j] == (uint32_t)p)
        {
          const size_t e = ((size_t)p * cap + j) * s * s + d * s + d;
          diag           = PER_COL ? values[e * ld_m + col] : values[e];
        }
    dinv[w] = diag != 0.0 ? 1.0 / diag : 1.0;
  }

  // x = 0, r = rhs, z = D^-1 r, p = z; partials of r.z (parity 0) and r.r
  template <bool PER_COL>
  __global__ __launch_bounds__(LOD_BLOCK) void k_mcg_init(int nrow, int n_rhs, int ngroup, const double *rhs, size_t ld_rhs,
                                                         double *x, size_t ld_x, McgVectors V)
  {
    __shared__ double b_rz[LOD_ROWS][LOD_COLS], b_rr[LOD_ROWS][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    a = 0.0, b = 0.0;
            if (i < nrow)
              {
                const size_t w = (size_t)i * n_rhs + col;
                const double f = rhs[(size_t)i * ld_rhs + col], zi = V.dinv[PER_COL ? w : (size_t)i] * f;
                x[(size_t)i * ld_x + col] = 0.0;
                V.r[w]                    = f;
                V.z[w]                    = zi;
                V.p[w]                    = zi;
                a                         = f * zi;
                b                         = f * f;
              }
            b_rz[lr][c] = a;
            b_rr[lr][c] = b;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb)
          {
            const size_t at = (size_t)g * n_rhs + c0 + threadIdx.x;
            V.rz[0][at]     = slod_lod_group_sum(b_rz, threadIdx.x);
            V.rr[at]        = slod_lod_group_sum(b_rr, threadIdx.x);
          }
        __syncthreads();
      }
  }

  // Y = A P on the block rows for the active columns; partials of p.Ap
  template <bool PER_COL>
  __global__ __launch_bounds__(LOD_BLOCK) void k_mcg_spmv(int nrow, int s, int cap, int NP, int n_rhs, int ngroup,
                                                         const double *__restrict__ values, size_t ld_m,
                                                         const uint32_t *__restrict__ cols, McgVectors V)
  {
    __shared__ double b_pAp[LOD_ROWS][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    prod = 0.0;
            if (i < nrow && V.active[col])
              {
                const double acc = slod_lod_row_product<PER_COL>(i, s, cap, NP, values, cols, V.p, (size_t)n_rhs, col, ld_m);
                const size_t w = (size_t)i * n_rhs + col;
                V.Ap[w]        = acc;
                prod           = acc * V.p[w];
              }
            b_pAp[lr][c] = prod;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb && V.active[c0 + threadIdx.x])
          V.pAp[(size_t)g * n_rhs + c0 + threadIdx.x] = slod_lod_group_sum(b_pAp, threadIdx.x);
        __syncthreads();
      }
  }

  // alpha = r.z / p.Ap from the partials; x += alpha p, r -= alpha Ap, z = D^-1 r; partials of the new r.z
  // (parity par ^ 1) and of r.r
  template <bool PER_COL>
  __global__ __launch_bounds__(LOD_BLOCK) void k_mcg_update_xr(int nrow, int n_rhs, int ngroup, int par, double *x, size_t ld_x,
                                                              McgVectors V)
  {
    __shared__ double b_rz[LOD_ROWS][LOD_COLS], b_rr[LOD_ROWS][LOD_COLS], s_sum[2][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // wave 0 sums the partials of p.Ap, wave 1 those of r.z, both in ascending group order
    if (wave < 2 && lane < nb && V.active[c0 + lane])
      s_sum[wave][lane] = slod_lod_ordered_sum(wave == 0 ? V.pAp : V.rz[par], ngroup, n_rhs, c0 + lane);
    __syncthreads();
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    a = 0.0, b = 0.0;
            if (i < nrow && V.active[col])
              {
                const double pAp = s_sum[0][c], alpha = pAp != 0.0 ? s_sum[1][c] / pAp : 0.0;
                const size_t w = (size_t)i * n_rhs + col, xi = (size_t)i * ld_x + col;
                const double ri = fma(-alpha, V.Ap[w], V.r[w]), zi = V.dinv[PER_COL ? w : (size_t)i] * ri;
                x[xi]  = fma(alpha, V.p[w], x[xi]);
                V.r[w] = ri;
                V.z[w] = zi;
                a      = ri * zi;
                b      = ri * ri;
              }
            b_rz[lr][c] = a;
            b_rr[lr][c] = b;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb && V.active[c0 + threadIdx.x])
          {
            const size_t at   = (size_t)g * n_rhs + c0 + threadIdx.x;
            V.rz[par ^ 1][at] = slod_lod_group_sum(b_rz, threadIdx.x);
            V.rr[at]          = slod_lod_group_sum(b_rr, threadIdx.x);
          }
        __syncthreads();
      }
  }

  // beta = r.z_new / r.z from the partials of both parities; p = z + beta p
  __global__ __launch_bounds__(LOD_BLOCK) void k_mcg_update_p(int nrow, int n_rhs, int ngroup, int par, McgVectors V)
  {
    __shared__ double s_sum[2][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2 && lane < nb && V.active[c0 + lane])
      s_sum[wave][lane] = slod_lod_ordered_sum(V.rz[wave == 0 ? par : par ^ 1], ngroup, n_rhs, c0 + lane);
    __syncthreads();
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
        {
          const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
          if (i < nrow && V.active[col])
            {
              const double rz = s_sum[0][c], beta = rz != 0.0 ? s_sum[1][c] / rz : 0.0;
              const size_t w = (size_t)i * n_rhs + col;
              V.p[w]         = fma(beta, V.p[w], V.z[w]);
            }
        }
  }

  // One thread per column: r.r from its partials.  first: it is ||rhs||^2, every column starts active.  A
  // column with r.r <= tol^2 ||rhs||^2 is frozen (a zero column at once: 0 iterations, residual 0).
  __global__ void k_mcg_check(int n_rhs, int ngroup, double tol2, int first, McgVectors V)
  {
    const int col = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (col >= n_rhs || (!first && !V.active[col]))
      return;
    const double rr = slod_lod_ordered_sum(V.rr, ngroup, n_rhs, col);
    if (first)
      V.rhs2[col] = rr;
    V.rr_last[col] = rr;
    V.active[col]  = rr <= tol2 * V.rhs2[col] ? 0 : 1;
  }
} // namespace

// The pieces of the workspace of one solve: 4 vectors, D^-1 (per_col: one per column), 4 partial arrays, 2 per-column
// scalars.
static McgVectors mcg_carve(SlodCarver &c, const LodShape &w, int n_rhs, bool per_col)
{
  const size_t nvec = (size_t)w.nrow * n_rhs, npart = (size_t)w.ngroup * n_rhs;
  McgVectors   V{};
  V.r = c.take(nvec), V.z = c.take(nvec), V.p = c.take(nvec), V.Ap = c.take(nvec);
  V.dinv = c.take(per_col ? nvec : (size_t)w.nrow);
  V.pAp = c.take(npart), V.rz[0] = c.take(npart), V.rz[1] = c.take(npart), V.rr = c.take(npart);
  V.rhs2 = c.take((size_t)n_rhs), V.rr_last = c.take((size_t)n_rhs); // read back in one copy
  return V;
}

void SlodLodWork::take_solve(SlodCarver &c, const slod_handle *h, bool matrix_per_column)
{
  per_col = matrix_per_column;
  cg      = mcg_carve(c, lod_shape(h, (int)its.size()), (int)its.size(), per_col).r;
}

namespace
{
  // The launches of one solve that touch the matrix or D^-1, for one value of PER_COL
  struct McgKernels
  {
    decltype(&k_mcg_diag<false>)      diag;
    decltype(&k_mcg_init<false>)      init;
    decltype(&k_mcg_spmv<false>)      spmv;
    decltype(&k_mcg_update_xr<false>) update_xr;
  };
  template <bool PER_COL>
  constexpr McgKernels mcg_kernels()
  {
    return {k_mcg_diag<PER_COL>, k_mcg_init<PER_COL>, k_mcg_spmv<PER_COL>, k_mcg_update_xr<PER_COL>};
  }
} // namespace

// The solve of slod_lod_solve_multi on a workspace the caller owns, so that a time loop allocates once.
hipError_t SlodLodWork::solve(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_rhs, size_t ld_rhs,
                              double *d_u, size_t ld_u, double rel_tol, int max_iterations, size_t ld_m)
{
  hipStream_t    st = h->stream;
  const int      n_rhs = (int)its.size();
  int           *d_active = active.get();
  const LodShape w = lod_shape(h, n_rhs);
  const int      s = w.s, cap = w.cap, NP = w.NP, nrow = w.nrow, ngroup = w.ngroup;
  const dim3     grid = lod_grid(w, SOLVE_MAX_BLOCKS), block(LOD_BLOCK);
  std::vector<int> flags((size_t)n_rhs, 1);
  std::fill(its.begin(), its.end(), 0);
  int        it = 0;
  SlodCarver hand{cg};
  McgVectors V = mcg_carve(hand, w, n_rhs, per_col);
  const McgKernels K = per_col ? mcg_kernels<true>() : mcg_kernels<false>();
  V.active     = d_active;
  const double tol2 = rel_tol * rel_tol;
  const dim3   ncheck = lod_flat_grid((size_t)n_rhs);
  hipLaunchKernelGGL(K.diag, lod_flat_grid(per_col ? (size_t)nrow * n_rhs : (size_t)nrow), block, 0, st, nrow, s, cap, n_rhs,
                     d_values, ld_m, d_cols, V.dinv);
  hipLaunchKernelGGL(K.init, grid, block, 0, st, nrow, n_rhs, ngroup, d_rhs, ld_rhs, d_u, ld_u, V);
  hipLaunchKernelGGL(k_mcg_check, ncheck, block, 0, st, n_rhs, ngroup, tol2, 1, V);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(flags.data(), d_active, (size_t)n_rhs * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  std::vector<int> was_active = flags;
  bool             any = e == hipSuccess && std::find(flags.begin(), flags.end(), 1) != flags.end();
  while (e == hipSuccess && any && it < max_iterations)
    {
      // a few iterations per convergence check: the scalars stay on the device in between
      const int burst = std::min(8, max_iterations - it);
      for (int b = 0; b < burst; ++b)
        {
          const int par = (it + b) & 1;
          hipLaunchKernelGGL(K.spmv, grid, block, 0, st, nrow, s, cap, NP, n_rhs, ngroup, d_values, ld_m, d_cols, V);
          hipLaunchKernelGGL(K.update_xr, grid, block, 0, st, nrow, n_rhs, ngroup, par, d_u, ld_u, V);
          hipLaunchKernelGGL(k_mcg_update_p, grid, block, 0, st, nrow, n_rhs, ngroup, par, V);
        }
      it += burst;
      hipLaunchKernelGGL(k_mcg_check, ncheck, block, 0, st, n_rhs, ngroup, tol2, 0, V);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(flags.data(), d_active, (size_t)n_rhs * sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess)
        e = hipStreamSynchronize(st);
      // a column that was active during the burst has done `it` iterations, frozen now or not
      for (int c = 0; c < n_rhs && e == hipSuccess; ++c)
        if (was_active[c])
          its[c] = it;
      was_active = flags;
      any        = e == hipSuccess && std::find(flags.begin(), flags.end(), 1) != flags.end();
    }
  std::vector<double> sc(2 * (size_t)n_rhs);
  if (e == hipSuccess)
    e = hipMemcpyAsync(sc.data(), V.rhs2, sc.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  if (e != hipSuccess)
    return e;
  for (int c = 0; c < n_rhs; ++c)
    res[c] = sc[c] > 0.0 ? std::sqrt(sc[(size_t)n_rhs + c] / sc[c]) : 0.0;
  last  = *std::max_element(its.begin(), its.end());
  worst = std::max(worst, last);
  return e;
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_solve_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_rhs, size_t ld_rhs,
                         int n_rhs, double *d_u, size_t ld_u, double rel_tol, int max_iterations, int *iterations,
                         double *rel_residual)
{
  if (!h || !d_values || !d_cols || !d_rhs || !d_u)
    return SLOD_ERR_ARGUMENT;
  if (n_rhs < 1 || max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_solve_multi: n_rhs < 1 or max_iterations < 0");
  if (const int rc = slod_check_ld(h, "slod_lod_solve_multi", "n_rhs", n_rhs, {ld_rhs, ld_u}))
    return rc;
  if (const int rc = slod_enter(h, nullptr, nullptr))
    return rc;
  // workspace allocated per call; the solve synchronises the stream before it returns
  SlodLodWork work;
  hipError_t  e = work.alloc(n_rhs, [&](SlodCarver &c) { work.take_solve(c, h); });
  if (e == hipSuccess)
    e = work.solve(h, d_values, d_cols, d_rhs, ld_rhs, d_u, ld_u, rel_tol, max_iterations);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_lod_solve_multi");
  work.report(iterations, rel_residual);
  return work.last;
}

} // extern "C"
#pragma GCC visibility pop
