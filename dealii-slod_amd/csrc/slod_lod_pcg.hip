// slod_lod_solve_multi_precond / slod_lod_solve_ensemble_precond: CG on the LOD space preconditioned by a banded factor
// the caller built (slod_lod_factor.hip) -- of the matrix before a local coefficient change, of one member of an
// ensemble, of the step matrix of another dt, or of the matrix itself (iterative refinement).  The reference has no
// counterpart (it runs CG + SSOR once, LOD.cc:990-998).
//
// The recurrence of slod_lod_multi.hip with  z = P^-1 r  where  z = D^-1 r  stands: every column has scalars of its own,
// the tiling and every summation order are those of slod_lod_tile.hip.h (one partial per (group, column), summed in
// ascending group order by every block that needs the scalar: no atomics, no grid barrier).  An iteration is five
// launches for all columns:
//   k_factor_solve   z = P^-1 r, out of place (slod_lod_factor_solve_launch: all columns on the factor's one member, or
//                    column k on member k)
//   k_pcg_dot        the stop rule of the iteration from the partials of r.r; partials of r.z (parity it & 1)
//   k_pcg_update_p   beta = r.z_new / r.z_old;  p = z + beta p  (the first iteration: p = z)
//   k_pcg_spmv       Ap = A p, partials of p.Ap
//   k_pcg_update_xr  alpha = r.z / p.Ap;  x += alpha p, r -= alpha Ap; partials of r.r
// Every boundary between two of them is a sum over all rows of a column or a product that reads p of other rows: a
// fusion across one would need a grid barrier.  What is fused is the check: there is no kernel of one thread per column.
//
// The stop rule runs on the device in every iteration (k_pcg_dot): a column with r.r <= rel_tol^2 ||rhs||^2 clears its
// active word, any other column counts the iteration it is about to run.  A frozen column is never written again (x, r,
// p, its partials, its counter; z is rewritten by the factor solve with the same words).  The host only reads the
// active words back every PCG_BURST iterations to decide whether to go on launching; nothing computed depends on it.
//
// A scalar of a column is summed by every block for itself from the same partials, so all blocks decide alike; the words
// of a column (active, counter, status, r.r) are written by block x = 0 of the column's chunk only.  A block reads the
// active word once: if it still reads 1 where block 0 has already cleared it, it reaches the decision of block 0 by its
// own sum and skips the column as well.
#include "slod_lod_tile.hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

namespace
{
  constexpr int PCG_MAX_BLOCKS = 256; // blocks per chunk, as SOLVE_MAX_BLOCKS
  constexpr int PCG_BURST      = 4;   // iterations between two read-backs of the active words

  enum { PCG_OK = 0, PCG_BAD_PAP = 1, PCG_BAD_RR = 2 }; // the status word of a column

  struct PcgVectors
  {
    double *r, *z, *p, *Ap;        // [nrow][n_rhs]
    double *pAp, *rz[2], *rr;      // partials [ngroup][n_rhs]
    double *rhs2, *rr_last, *bad;  // [n_rhs] each, read back in one copy: ||rhs||^2, the last r.r, the value of a breakdown
    int    *iters, *status;        // [n_rhs] each, read back in one copy
    int    *active;                // [n_rhs]
  };

  // x = 0, r = rhs; partials of r.r; every column active, counter and status 0
  __global__ __launch_bounds__(LOD_BLOCK) void k_pcg_init(int nrow, int n_rhs, int ngroup, const double *rhs, size_t ld_rhs, double *x,
                                                         size_t ld_x, PcgVectors V)
  {
    __shared__ double b_rr[LOD_ROWS][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    if (blockIdx.x == 0 && (int)threadIdx.x < nb)
      {
        const int col  = c0 + threadIdx.x;
        V.active[col]  = 1;
        V.iters[col]   = 0;
        V.status[col]  = PCG_OK;
        V.bad[col]     = 0.0;
        V.rhs2[col]    = 0.0;
        V.rr_last[col] = 0.0;
      }
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    b = 0.0;
            if (i < nrow)
              {
                const double f = rhs[(size_t)i * ld_rhs + col];
                x[(size_t)i * ld_x + col]     = 0.0;
                V.r[(size_t)i * n_rhs + col] = f;
                b                            = f * f;
              }
            b_rr[lr][c] = b;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb)
          V.rr[(size_t)g * n_rhs + c0 + threadIdx.x] = slod_lod_group_sum(b_rr, threadIdx.x);
        __syncthreads();
      }
  }

  // The stop rule of an iteration, then the partials of r.z (parity par) for the columns that go on.  first: r is the
  // right-hand side, r.r is ||rhs||^2.  last: max_iterations is reached: the rule only, nothing is counted.
  __global__ __launch_bounds__(LOD_BLOCK) void k_pcg_dot(int nrow, int n_rhs, int ngroup, int par, int first, int last, double tol2,
                                                        PcgVectors V)
  {
    __shared__ double b_rz[LOD_ROWS][LOD_COLS];
    __shared__ int    s_go[LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    if ((int)threadIdx.x < LOD_COLS)
      {
        const int col = c0 + threadIdx.x;
        int       go  = 0;
        if ((int)threadIdx.x < nb && V.active[col])
          {
            const double rr = slod_lod_ordered_sum(V.rr, ngroup, n_rhs, col), rhs2 = first ? rr : V.rhs2[col];
            const bool   finite = rr < HUGE_VAL; // false for NaN too
            const bool   stop = rr <= tol2 * rhs2;
            go                = finite && !stop;
            if (blockIdx.x == 0)
              {
                if (first)
                  V.rhs2[col] = rr;
                V.rr_last[col] = rr;
                if (!finite)
                  {
                    V.status[col] = PCG_BAD_RR;
                    V.bad[col]    = rr;
                  }
                if (!go)
                  V.active[col] = 0;
                else if (!last)
                  V.iters[col] += 1;
              }
          }
        s_go[threadIdx.x] = go;
      }
    __syncthreads();
    if (last)
      return;
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    a = 0.0;
            if (i < nrow && s_go[c])
              {
                const size_t w = (size_t)i * n_rhs + col;
                a              = V.r[w] * V.z[w];
              }
            b_rz[lr][c] = a;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb && s_go[threadIdx.x])
          V.rz[par][(size_t)g * n_rhs + c0 + threadIdx.x] = slod_lod_group_sum(b_rz, threadIdx.x);
        __syncthreads();
      }
  }

  // beta = r.z_new / r.z_old from the partials of both parities; p = z + beta p.  first: p = z
  __global__ __launch_bounds__(LOD_BLOCK) void k_pcg_update_p(int nrow, int n_rhs, int ngroup, int par, int first, PcgVectors V)
  {
    __shared__ double s_sum[2][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // wave 0 sums the partials of the new r.z, wave 1 those of the old one (nobody writes an active word here)
    if (!first && wave < 2 && lane < nb && V.active[c0 + lane])
      s_sum[wave][lane] = slod_lod_ordered_sum(V.rz[wave == 0 ? par : par ^ 1], ngroup, n_rhs, c0 + lane);
    __syncthreads();
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
        {
          const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
          if (i < nrow && V.active[col])
            {
              const size_t w = (size_t)i * n_rhs + col;
              if (first)
                V.p[w] = V.z[w];
              else
                {
                  const double rz = s_sum[1][c], beta = rz != 0.0 ? s_sum[0][c] / rz : 0.0;
                  V.p[w]          = fma(beta, V.p[w], V.z[w]);
                }
            }
        }
  }

  // Ap = A p on the block rows for the active columns; partials of p.Ap.  PER_COL: column k reads matrix k of an
  // ensemble matrix, ld_m apart
  template <bool PER_COL>
  __global__ __launch_bounds__(LOD_BLOCK) void k_pcg_spmv(int nrow, int s, int cap, int NP, int n_rhs, int ngroup,
                                                         const double *__restrict__ values, size_t ld_m,
                                                         const uint32_t *__restrict__ cols, PcgVectors V)
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

  // alpha = r.z / p.Ap from the partials; x += alpha p, r -= alpha Ap; partials of the new r.r.  A column whose p.Ap is
  // not > 0 (an indefinite matrix, NaN) sets its status and freezes where it stands.
  __global__ __launch_bounds__(LOD_BLOCK) void k_pcg_update_xr(int nrow, int n_rhs, int ngroup, int par, double *x, size_t ld_x,
                                                              PcgVectors V)
  {
    __shared__ double b_rr[LOD_ROWS][LOD_COLS], s_sum[2][LOD_COLS];
    __shared__ int    s_go[LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((int)threadIdx.x < LOD_COLS)
      s_go[threadIdx.x] = (int)threadIdx.x < nb && V.active[c0 + threadIdx.x]; // read once
    __syncthreads();
    // wave 0 sums the partials of p.Ap, wave 1 those of r.z, both in ascending group order
    if (wave < 2 && s_go[lane])
      s_sum[wave][lane] = slod_lod_ordered_sum(wave == 0 ? V.pAp : V.rz[par], ngroup, n_rhs, c0 + lane);
    __syncthreads();
    if ((int)threadIdx.x < LOD_COLS && s_go[threadIdx.x])
      {
        const double pAp = s_sum[0][threadIdx.x];
        if (!(pAp > 0.0)) // false for NaN too
          {
            s_go[threadIdx.x] = 0;
            if (blockIdx.x == 0)
              {
                const int col = c0 + threadIdx.x;
                V.status[col] = PCG_BAD_PAP;
                V.bad[col]    = pAp;
                V.active[col] = 0;
              }
          }
      }
    __syncthreads();
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    b = 0.0;
            if (i < nrow && s_go[c])
              {
                // (the guard of k_mcg_update_xr, kept as the rule of these kernels: a column that gets here has p.Ap > 0)
                const double pAp = s_sum[0][c], alpha = pAp != 0.0 ? s_sum[1][c] / pAp : 0.0;
                const size_t w = (size_t)i * n_rhs + col, xi = (size_t)i * ld_x + col;
                const double ri = fma(-alpha, V.Ap[w], V.r[w]);
                x[xi]  = fma(alpha, V.p[w], x[xi]);
                V.r[w] = ri;
                b      = ri * ri;
              }
            b_rr[lr][c] = b;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb && s_go[threadIdx.x])
          V.rr[(size_t)g * n_rhs + c0 + threadIdx.x] = slod_lod_group_sum(b_rr, threadIdx.x);
        __syncthreads();
      }
  }

  // The pieces of the workspace of one solve: 4 vectors, 4 partial arrays, 3 per-column scalars, 2 per-column words
  PcgVectors pcg_carve(SlodCarver &c, const LodShape &w, int n_rhs)
  {
    const size_t nvec = (size_t)w.nrow * n_rhs, npart = (size_t)w.ngroup * n_rhs;
    PcgVectors   V{};
    V.r = c.take(nvec), V.z = c.take(nvec), V.p = c.take(nvec), V.Ap = c.take(nvec);
    V.pAp = c.take(npart), V.rz[0] = c.take(npart), V.rz[1] = c.take(npart), V.rr = c.take(npart);
    V.rhs2 = c.take((size_t)n_rhs), V.rr_last = c.take((size_t)n_rhs), V.bad = c.take((size_t)n_rhs); // read back in one copy
    V.iters  = (int *)c.take((size_t)n_rhs); // 2 n_rhs words in n_rhs doubles, read back in one copy
    V.status = V.iters ? V.iters + n_rhs : nullptr;
    return V;
  }
} // namespace

void SlodLodWork::take_precond(SlodCarver &c, const slod_handle *h)
{
  pcg = pcg_carve(c, lod_shape(h, (int)its.size()), (int)its.size()).r;
}

// The solve of slod_lod_solve_multi_precond / _ensemble_precond on a workspace the caller owns.
hipError_t SlodLodWork::solve_precond(slod_handle *h, const slod_lod_factor *f, const double *d_values, const uint32_t *d_cols,
                                      const double *d_rhs, size_t ld_rhs, double *d_u, size_t ld_u, double rel_tol, int max_iterations,
                                      bool matrix_per_column, size_t ld_m)
{
  hipStream_t    st = h->stream;
  const int      n_rhs = (int)its.size();
  const LodShape w = lod_shape(h, n_rhs);
  const int      s = w.s, cap = w.cap, NP = w.NP, nrow = w.nrow, ngroup = w.ngroup;
  const dim3     grid = lod_grid(w, PCG_MAX_BLOCKS), block(LOD_BLOCK), cols_only((unsigned)1, (unsigned)w.nchunk);
  SlodCarver     hand{pcg};
  PcgVectors     V = pcg_carve(hand, w, n_rhs);
  V.active         = active.get();
  const double   tol2 = rel_tol * rel_tol;
  const bool     member_per_column = f->n_members > 1; // else all columns on the factor's one member
  std::vector<int> flags((size_t)n_rhs, 1);
  bad_col = -1;
  hipLaunchKernelGGL(k_pcg_init, grid, block, 0, st, nrow, n_rhs, ngroup, d_rhs, ld_rhs, d_u, ld_u, V);
  hipError_t e = hipGetLastError();
  int        it = 0;
  bool       any = true;
  while (e == hipSuccess && any && it < max_iterations)
    {
      // a few iterations per read-back of the active words: the stop rule itself runs on the device in every one
      const int burst = std::min(PCG_BURST, max_iterations - it);
      for (int b = 0; b < burst; ++b, ++it)
        {
          const int par = it & 1, first = it == 0;
          if (member_per_column)
            slod_lod_factor_solve_launch(f, st, V.r, (size_t)n_rhs, 1, V.z, (size_t)n_rhs, 0, n_rhs);
          else
            slod_lod_factor_solve_launch(f, st, V.r, (size_t)n_rhs, n_rhs, V.z, (size_t)n_rhs);
          hipLaunchKernelGGL(k_pcg_dot, grid, block, 0, st, nrow, n_rhs, ngroup, par, first, 0, tol2, V);
          hipLaunchKernelGGL(k_pcg_update_p, grid, block, 0, st, nrow, n_rhs, ngroup, par, first, V);
          if (matrix_per_column)
            hipLaunchKernelGGL(k_pcg_spmv<true>, grid, block, 0, st, nrow, s, cap, NP, n_rhs, ngroup, d_values, ld_m, d_cols, V);
          else
            hipLaunchKernelGGL(k_pcg_spmv<false>, grid, block, 0, st, nrow, s, cap, NP, n_rhs, ngroup, d_values, ld_m, d_cols, V);
          hipLaunchKernelGGL(k_pcg_update_xr, grid, block, 0, st, nrow, n_rhs, ngroup, par, d_u, ld_u, V);
        }
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(flags.data(), V.active, (size_t)n_rhs * sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess)
        e = hipStreamSynchronize(st);
      any = e == hipSuccess && std::find(flags.begin(), flags.end(), 1) != flags.end();
    }
  // the rule on the residual of the last iteration (max_iterations reached), or of none (max_iterations = 0)
  if (e == hipSuccess && any)
    {
      hipLaunchKernelGGL(k_pcg_dot, cols_only, block, 0, st, nrow, n_rhs, ngroup, 0, it == 0, 1, tol2, V);
      e = hipGetLastError();
    }
  std::vector<double> sc(3 * (size_t)n_rhs);
  std::vector<int>    words(2 * (size_t)n_rhs);
  if (e == hipSuccess)
    e = hipMemcpyAsync(sc.data(), V.rhs2, sc.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(words.data(), V.iters, words.size() * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  if (e != hipSuccess)
    {
      (void)hipStreamSynchronize(st); // nothing may still run on the workspace when its owner frees it
      return e;
    }
  for (int c = 0; c < n_rhs; ++c)
    {
      its[c] = words[c];
      res[c] = sc[c] > 0.0 ? std::sqrt(sc[(size_t)n_rhs + c] / sc[c]) : 0.0;
      if (words[(size_t)n_rhs + c] != PCG_OK && bad_col < 0)
        {
          bad_col   = c;
          bad_it    = words[c];
          bad_pAp   = words[(size_t)n_rhs + c] == PCG_BAD_PAP;
          bad_value = sc[2 * (size_t)n_rhs + c];
        }
    }
  last  = *std::max_element(its.begin(), its.end());
  worst = std::max(worst, last);
  return e;
}

namespace
{
  // What both calls check of the preconditioner, and the solve.  columns: "column" or "member", for the text of a breakdown
  int precond_solve(slod_handle *h, const char *who, const char *columns, slod_lod_factor *f_P, int f_members, const double *d_values,
                    size_t ld_m, bool matrix_per_column, const uint32_t *d_cols, const double *d_rhs, size_t ld_rhs, int n, double *d_u,
                    size_t ld_u, double rel_tol, int max_iterations, int *iterations, double *rel_residual)
  {
    if (const int rc = slod_lod_factor_check(h, who, f_P, f_members))
      return rc;
    if (f_P->kind == SLOD_FACTOR_LDL && !(f_P->min_pivot > 0.0))
      return slod_fail(h, SLOD_ERR_ARGUMENT,
                       std::string(who) + ": the preconditioner must be positive definite: this LDL^T factor has a pivot that is not > 0");
    if (const int rc = slod_enter(h, nullptr, nullptr))
      return rc;
    // workspace allocated per call; the solve synchronises the stream before it returns, on every path
    SlodLodWork work;
    hipError_t  e = work.alloc(n, [&](SlodCarver &c) { work.take_precond(c, h); });
    if (e == hipSuccess)
      e = work.solve_precond(h, f_P, d_values, d_cols, d_rhs, ld_rhs, d_u, ld_u, rel_tol, max_iterations, matrix_per_column, ld_m);
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who);
    work.report(iterations, rel_residual);
    if (work.bad_col >= 0)
      {
        char msg[240];
        if (work.bad_pAp)
          std::snprintf(msg, sizeof msg, "%s: %s %d, iteration %d: p.Ap = %g is not > 0: the matrix is not positive definite", who,
                        columns, work.bad_col, work.bad_it, work.bad_value);
        else
          std::snprintf(msg, sizeof msg, "%s: %s %d, iteration %d: r.r = %g is not finite", who, columns, work.bad_col, work.bad_it,
                        work.bad_value);
        return slod_fail(h, SLOD_ERR_NUMERIC, msg);
      }
    return work.last;
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_solve_multi_precond(slod_handle *h, slod_lod_factor *f_P, const double *d_values, const uint32_t *d_cols,
                                 const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u, size_t ld_u, double rel_tol,
                                 int max_iterations, int *iterations, double *rel_residual)
{
  const char *who = "slod_lod_solve_multi_precond";
  if (!h || !d_values || !d_cols || !d_rhs || !d_u)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  if (n_rhs < 1 || max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_rhs < 1 or max_iterations < 0");
  if (const int rc = slod_check_ld(h, who, "n_rhs", n_rhs, {ld_rhs, ld_u}))
    return rc;
  return precond_solve(h, who, "column", f_P, 1, d_values, 1, false, d_cols, d_rhs, ld_rhs, n_rhs, d_u, ld_u, rel_tol, max_iterations,
                       iterations, rel_residual);
}

int slod_lod_solve_ensemble_precond(slod_handle *h, slod_lod_factor *f_P, const double *d_values, size_t ld_m, const uint32_t *d_cols,
                                    const double *d_rhs, size_t ld_rhs, int n_members, double *d_u, size_t ld_u, double rel_tol,
                                    int max_iterations, int *iterations, double *rel_residual)
{
  const char *who = "slod_lod_solve_ensemble_precond";
  if (!h || !d_values || !d_cols || !d_rhs || !d_u)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  // (no cap on n_members: a factor of several members has at most 65535 and must have exactly n_members)
  if (n_members < 1 || max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or max_iterations < 0");
  if (const int rc = slod_check_ld(h, who, "n_members", n_members, {ld_m, ld_rhs, ld_u}))
    return rc;
  // a factor of one member is shared by all columns; else it must hold a member per column
  return precond_solve(h, who, "member", f_P, f_P && f_P->n_members == 1 ? 1 : n_members, d_values, ld_m, true, d_cols, d_rhs, ld_rhs,
                       n_members, d_u, ld_u, rel_tol, max_iterations, iterations, rel_residual);
}

} // extern "C"
#pragma GCC visibility pop
