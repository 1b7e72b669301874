// The L2 side of the coarse problem and a time loop on it (the reference has no counterpart: it solves one
// stationary problem, LOD.cc:976-1002):
//   slod_lod_mass_matrix     block rows of  M_LOD = C^T M_rho C  in the layout and pattern of slod_lod_matrix
//   slod_lod_apply_multi     Y = A X for any matrix in that layout, columns on lanes
//   slod_lod_matrix_combine  out = alpha A + beta B on two values arrays of one pattern
//   slod_lod_theta_steps     n_steps of the theta scheme for  M u' + A u = b(t), the state stays on the device
// The mass kernel is an L2/HBM-bound gather like k_lod_matrix (slod_lod_system.hip) and shares its index calculus
// (slod_grid.hip.h); the solve of a step is the recurrence of slod_lod_solve_multi (slod_lod_multi.hip) on a
// workspace this file owns for the whole loop.
#include "slod_lod_system.hip.h"
#include "slod_lod_tile.hip.h"

#include <algorithm>
#include <vector>

namespace
{
  // M_LOD block rows.  Block = one row patch p; the row is lod_mass_row (slod_lod_system.hip.h).
  template <int S>
  __global__ __launch_bounds__(256) void k_lod_mass(const SlodGrid G, const uint32_t *rows, const double *basis, size_t stride,
                                                   const double *rho, double scale, double *values, uint32_t *cols)
  {
    lod_mass_row<S>(G, rows[blockIdx.x], blockIdx.x, basis, stride, rho, scale, values, 1, cols);
  }

  // ---------------------------------------------------------------------------------
  // Y = A X on the block rows, the tiling and the row product of k_mcg_spmv (slod_lod_tile.hip.h): the bits of a
  // column depend on the matrix and that column.
  // ---------------------------------------------------------------------------------
  constexpr int APPLY_MAX_BLOCKS = 1024; // blocks per chunk

  __global__ __launch_bounds__(LOD_BLOCK) void k_lod_apply(int nrow, int s, int cap, int NP, int n_rhs, int ngroup,
                                                         const double *__restrict__ values, const uint32_t *__restrict__ cols,
                                                         const double *__restrict__ x, size_t ld_x, double *__restrict__ y,
                                                         size_t ld_y)
  {
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
        {
          const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
          if (i >= nrow)
            continue;
          const double acc = slod_lod_row_product(i, s, cap, NP, values, cols, x, ld_x, col);
          y[(size_t)i * ld_y + col] = acc;
        }
  }

  // out = alpha a + beta b per word (lod_combine_word, slod_lod_system.hip.h)
  __global__ __launch_bounds__(256) void k_lod_combine(size_t n, double alpha, const double *a, double beta, const double *b,
                                                      double *out)
  {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
      out[i] = lod_combine_word(alpha, a[i], beta, b[i]);
  }

  // g = dt (theta b1 + (1 - theta) b0 - g) per (row, column); g holds A u on entry.  b0 / b1 NULL: zero load.
  __global__ __launch_bounds__(256) void k_theta_rhs(int nrow, int n_rhs, double dt, double theta, const double *b0,
                                                    const double *b1, size_t ld_b, double *g)
  {
#pragma clang fp contract(off)
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (size_t)nrow * n_rhs)
      return;
    const size_t i = w / n_rhs, c = w - i * n_rhs;
    double       load = 0.0;
    if (b0)
      {
        const double t1 = theta * b1[i * ld_b + c], t0 = (1.0 - theta) * b0[i * ld_b + c];
        load            = t1 + t0;
      }
    g[w] = dt * (load - g[w]);
  }

  // u += delta
  __global__ __launch_bounds__(256) void k_theta_advance(int nrow, int n_rhs, const double *delta, double *u, size_t ld_u)
  {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (size_t)nrow * n_rhs)
      return;
    const size_t i = w / n_rhs, c = w - i * n_rhs;
    u[i * ld_u + c] += delta[w];
  }
} // namespace

// k_lod_apply for the other loops of the library (slod_lod_eig.hip); arguments are checked by the caller
void slod_lod_apply_launch(const slod_handle *h, hipStream_t st, const double *d_values, const uint32_t *d_cols, const double *d_x,
                           size_t ld_x, int n_rhs, double *d_y, size_t ld_y)
{
  const LodShape w = lod_shape(h, n_rhs);
  hipLaunchKernelGGL(k_lod_apply, lod_grid(w, APPLY_MAX_BLOCKS), dim3(LOD_BLOCK), 0, st, w.nrow, w.s, w.cap, w.NP, n_rhs, w.ngroup,
                     d_values, d_cols, d_x, ld_x, d_y, ld_y);
}

// k_lod_combine on n values for the other loops of the library (slod_lod_wave.hip)
void slod_lod_combine_launch(hipStream_t st, size_t n, double alpha, const double *d_a, double beta, const double *d_b, double *d_out)
{
  hipLaunchKernelGGL(k_lod_combine, lod_flat_grid(n), dim3(LOD_BLOCK), 0, st, n, alpha, d_a, beta, d_b, d_out);
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_mass_matrix(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, size_t stride,
                         const double *d_rho, double *d_values, uint32_t *d_cols, void *hip_stream)
{
  if (!h || (n_rows && (!rows || !d_basis || !d_values || !d_cols)))
    return SLOD_ERR_ARGUMENT;
  // (the ids are checked here as well as by the upload: a bad id is refused before any device work)
  if (const int rc = slod_check_rows(h, "slod_lod_mass_matrix", rows, n_rows))
    return rc;
  if (n_rows == 0)
    return SLOD_OK;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  SlodDevBuf<uint32_t> d_rows;
  if (const int rc = slod_upload_rows(h, "slod_lod_mass_matrix", rows, n_rows, st, &d_rows))
    return rc;
  const double hf = 1.0 / h->NE, scale = hf * hf / 36.0;
  if (h->cfg.spacedim == 1)
    hipLaunchKernelGGL(k_lod_mass<1>, dim3((unsigned)n_rows), dim3(256), 0, st, slod_grid_of(h), d_rows.get(), d_basis, stride,
                       d_rho, scale, d_values, d_cols);
  else
    hipLaunchKernelGGL(k_lod_mass<2>, dim3((unsigned)n_rows), dim3(256), 0, st, slod_grid_of(h), d_rows.get(), d_basis, stride,
                       d_rho, scale, d_values, d_cols);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); // d_rows is freed on return
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_mass_matrix");
}

int slod_lod_apply_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                         int n_rhs, double *d_y, size_t ld_y, void *hip_stream)
{
  if (!h || !d_values || !d_cols || !d_x || !d_y)
    return SLOD_ERR_ARGUMENT;
  if (n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_apply_multi: n_rhs < 1");
  if (const int rc = slod_check_ld(h, "slod_lod_apply_multi", "n_rhs", n_rhs, {ld_x, ld_y}))
    return rc;
  if (d_x == d_y)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_apply_multi: the product cannot run in place");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  slod_lod_apply_launch(h, st, d_values, d_cols, d_x, ld_x, n_rhs, d_y, ld_y);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_apply_multi");
}

int slod_lod_matrix_combine(slod_handle *h, double alpha, const double *d_a, double beta, const double *d_b, double *d_out,
                            void *hip_stream)
{
  if (!h || !d_a || !d_b || !d_out)
    return SLOD_ERR_ARGUMENT;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int s = h->cfg.spacedim;
  slod_lod_combine_launch(st, (size_t)h->NP * slod_lod_row_capacity(h) * s * s, alpha, d_a, beta, d_b, d_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_matrix_combine");
}

int slod_lod_theta_steps(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double dt,
                         double theta, int n_steps, int n_rhs, double *d_u, size_t ld_u, const double *d_load, size_t ld_load,
                         size_t load_step_stride, double rel_tol, int max_iterations, int *iterations, double *rel_residual)
{
  if (!h || !d_stiffness || !d_mass || !d_cols || !d_u)
    return SLOD_ERR_ARGUMENT;
  if (!(dt > 0.0) || !(theta >= 0.0 && theta <= 1.0))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]");
  if (n_steps < 1 || n_rhs < 1 || max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_theta_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0");
  if (const int rc = slod_check_ld(h, "slod_lod_theta_steps", "n_rhs", n_rhs, {ld_u, d_load ? ld_load : ld_u}))
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const LodShape w = lod_shape(h, n_rhs);
  const size_t   nmat = (size_t)w.NP * w.cap * w.s * w.s, nvec = (size_t)w.nrow * n_rhs;
  // one allocation for the whole loop: S, g, delta and the workspace of the solve
  double     *S, *g, *delta;
  SlodLodWork work;
  hipError_t  e = work.alloc(n_rhs, [&](SlodCarver &c) { S = c.take(nmat), g = c.take(nvec), delta = c.take(nvec), work.take_solve(c, h); });
  if (e == hipSuccess)
    {
      slod_lod_combine_launch(st, nmat, 1.0, d_mass, theta * dt, d_stiffness, S);
      e = hipGetLastError();
      for (int k = 0; k < n_steps && e == hipSuccess; ++k)
        {
          const double *b0 = d_load ? d_load + (size_t)k * load_step_stride : nullptr;
          const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
          slod_lod_apply_launch(h, st, d_stiffness, d_cols, d_u, ld_u, n_rhs, g, (size_t)n_rhs);
          hipLaunchKernelGGL(k_theta_rhs, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_rhs, dt, theta, b0, b1, ld_load, g);
          e = hipGetLastError();
          if (e == hipSuccess)
            e = work.solve(h, S, d_cols, g, (size_t)n_rhs, delta, (size_t)n_rhs, rel_tol, max_iterations);
          if (e != hipSuccess)
            break;
          work.record(k, iterations, rel_residual);
          hipLaunchKernelGGL(k_theta_advance, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_rhs, delta, d_u, ld_u);
          e = hipGetLastError();
        }
      if (e == hipSuccess)
        e = hipStreamSynchronize(st); // the workspace is freed on return
    }
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_lod_theta_steps");
  return work.worst;
}

// The loop of slod_lod_theta_steps with the factor's two sweeps in place of the CG recurrence: the whole loop is queued
// and the stream is waited for once.
int slod_lod_theta_steps_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const uint32_t *d_cols, double dt,
                                double theta, int n_steps, int n_rhs, double *d_u, size_t ld_u, const double *d_load, size_t ld_load,
                                size_t load_step_stride)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_stiffness || !d_cols || !d_u)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_theta_steps_direct: NULL matrix, d_cols or d_u");
  if (!(dt > 0.0) || !(theta >= 0.0 && theta <= 1.0))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]");
  if (n_steps < 1 || n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_theta_steps_direct: n_steps < 1 or n_rhs < 1");
  if (const int rc = slod_check_ld(h, "slod_lod_theta_steps_direct", "n_rhs", n_rhs, {ld_u, d_load ? ld_load : ld_u}))
    return rc;
  if (const int rc = slod_lod_factor_check(h, "slod_lod_theta_steps_direct", f_S)) // last: it reads the factor
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const LodShape     w = lod_shape(h, n_rhs);
  const size_t       nvec = (size_t)w.nrow * n_rhs;
  SlodDevBuf<double> work; // g, delta
  hipError_t         e = work.alloc(2 * nvec);
  if (e == hipSuccess)
    {
      double *g = work.get(), *delta = g + nvec;
      for (int k = 0; k < n_steps && e == hipSuccess; ++k)
        {
          const double *b0 = d_load ? d_load + (size_t)k * load_step_stride : nullptr;
          const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
          slod_lod_apply_launch(h, st, d_stiffness, d_cols, d_u, ld_u, n_rhs, g, (size_t)n_rhs);
          hipLaunchKernelGGL(k_theta_rhs, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_rhs, dt, theta, b0, b1, ld_load, g);
          slod_lod_factor_solve_launch(f_S, st, g, (size_t)n_rhs, n_rhs, delta, (size_t)n_rhs);
          hipLaunchKernelGGL(k_theta_advance, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_rhs, delta, d_u, ld_u);
          e = hipGetLastError();
        }
      const hipError_t es = hipStreamSynchronize(st); // the workspace is freed on return
      if (e == hipSuccess)
        e = es;
    }
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_theta_steps_direct");
}

// The loop of slod_lod_theta_steps_direct with a matrix and a factor per column: the product is k_ens_apply
// (slod_lod_ensemble.hip), the solve the member axis of k_factor_solve with one column per member; k_theta_rhs and
// k_theta_advance work per (row, column) and serve as they are.
int slod_lod_theta_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_m,
                                         const uint32_t *d_cols, double dt, double theta, int n_steps, int n_members, double *d_u,
                                         size_t ld_u, const double *d_load, size_t ld_load, size_t load_step_stride)
{
  const char *who = "slod_lod_theta_steps_ensemble_direct";
  if (!h || !d_stiffness || !d_cols || !d_u)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle, matrix, d_cols or d_u");
  if (!(dt > 0.0) || !(theta >= 0.0 && theta <= 1.0))
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": dt <= 0 or theta outside [0, 1]");
  if (n_steps < 1 || n_members < 1 || n_members > 65535)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_steps < 1, n_members < 1 or > 65535");
  if (const int rc = slod_check_ld(h, who, "n_members", n_members, {ld_m, ld_u, d_load ? ld_load : ld_u}))
    return rc;
  if (const int rc = slod_lod_factor_check(h, who, f_S, n_members)) // last: it reads the factor
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const LodShape     w = lod_shape(h, n_members);
  const size_t       nvec = (size_t)w.nrow * n_members;
  SlodDevBuf<double> work; // g, delta
  hipError_t         e = work.alloc(2 * nvec);
  if (e == hipSuccess)
    {
      double *g = work.get(), *delta = g + nvec;
      for (int k = 0; k < n_steps && e == hipSuccess; ++k)
        {
          const double *b0 = d_load ? d_load + (size_t)k * load_step_stride : nullptr;
          const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
          slod_lod_apply_ensemble_launch(h, st, d_stiffness, ld_m, d_cols, d_u, ld_u, n_members, g, (size_t)n_members);
          hipLaunchKernelGGL(k_theta_rhs, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_members, dt, theta, b0, b1, ld_load, g);
          slod_lod_factor_solve_launch(f_S, st, g, (size_t)n_members, 1, delta, (size_t)n_members, 0, n_members);
          hipLaunchKernelGGL(k_theta_advance, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_members, delta, d_u, ld_u);
          e = hipGetLastError();
        }
      const hipError_t es = hipStreamSynchronize(st); // the workspace is freed on return
      if (e == hipSuccess)
        e = es;
    }
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

} // extern "C"
#pragma GCC visibility pop
