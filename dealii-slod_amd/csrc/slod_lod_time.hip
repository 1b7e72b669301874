// The L2 side of the coarse problem and a time loop on it (the reference has no counterpart: it solves one
// stationary problem, LOD.cc:976-1002):
//   slod_lod_mass_matrix     block rows of  M_LOD = C^T M_rho C  in the layout and pattern of slod_lod_matrix
//   slod_lod_apply_multi     Y = A X for any matrix in that layout, columns on lanes
//   slod_lod_matrix_combine  out = alpha A + beta B on two values arrays of one pattern
//   slod_lod_theta_steps     n_steps of the theta scheme for  M u' + A u = b(t), the state stays on the device
// and slod_lod_theta_steps_direct / _ensemble_direct, the same loop on a factor the caller built (slod_lod_factor.hip),
// for one matrix or with a matrix, a factor and a column per member.
// The mass kernel is an L2/HBM-bound gather like k_lod_matrix (slod_lod_system.hip) and shares its index calculus
// (slod_grid.hip.h).  The loop is written once (theta_steps) on the operator of a column and the solve of a step
// (SlodLodOperator, SlodLodStepSolve, slod_host.h): the recurrence of slod_lod_solve_multi (slod_lod_multi.hip) on a
// workspace the loop owns, or the two sweeps of the factor; the argument checks of the three calls are theta_check.
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

namespace
{
  // The argument checks of the three theta calls, in one order; every call keeps its wording.  arrays: no array is NULL;
  // n: n_rhs or n_members; lds: the leading dimensions of the vectors.  The factor is looked at last: only that check
  // reads it.
  int theta_check(const slod_handle *h, const std::string &who, const SlodLodStepSolve &solve, const SlodLodOperator &A, bool arrays,
                  double dt, double theta, int n_steps, int n, std::initializer_list<size_t> lds)
  {
    const bool cg = solve.cg(), ens = A.per_col;
    if (!ens && (!h || (cg && !arrays)))
      return SLOD_ERR_ARGUMENT;
    if (!h || !arrays)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (ens ? ": NULL handle, matrix, d_cols or d_u" : ": NULL matrix, d_cols or d_u"));
    if (!(dt > 0.0) || !(theta >= 0.0 && theta <= 1.0))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": dt <= 0 or theta outside [0, 1]");
    if (n_steps < 1 || n < 1 || (ens && n > 65535) || (cg && solve.max_iterations < 0))
      return slod_fail(h, SLOD_ERR_ARGUMENT,
                       who + (cg    ? ": n_steps < 1, n_rhs < 1 or max_iterations < 0"
                              : ens ? ": n_steps < 1, n_members < 1 or > 65535"
                                    : ": n_steps < 1 or n_rhs < 1"));
    if (const int rc = slod_check_ld_of(h, who.c_str(), ens, {A.ld_m}, n, lds))
      return rc;
    return cg ? SLOD_OK : slod_lod_factor_check(h, who.c_str(), solve.f, ens ? n : 1);
  }

  // n_steps of the theta scheme on n columns,  S delta = dt (theta b1 + (1 - theta) b0 - A u),  u += delta,  whatever
  // solves the step; the body of the three calls.  CG: S = M + theta dt A is built here and every solve synchronises; on a
  // factor (of that S) the whole loop is queued and the stream is waited for once.  Returns the largest iteration count
  // of a step (0 on a factor) or a negative status.  A record armed on the handle (SlodLodRecord, slod_host.h) is taken
  // first, checked after the call's own checks and queued on st: u at the receivers after the entry state and every
  // every-th advance.  A source armed on it (SlodLodSource) is taken with the record, checked after it, and adds one
  // product a step, whose two vectors the right-hand side reads in place of the loads.
  int theta_steps(slod_handle *h, const char *who, SlodLodStepSolve &&solve, const SlodLodOperator &A, const double *d_mass,
                  const uint32_t *d_cols, double dt, double theta, int n_steps, int n, double *d_u, size_t ld_u, const double *d_load,
                  size_t ld_load, size_t load_step_stride)
  {
    SlodLodRecord rec = slod_lod_record_take(h);
    SlodLodSource src = slod_lod_source_take(h);
    if (const int rc = theta_check(h, who, solve, A, A.values && (d_mass || !solve.cg()) && d_cols && d_u, dt, theta, n_steps, n,
                                   {ld_u, d_load ? ld_load : ld_u}))
      return rc;
    if (const int rc = slod_lod_record_check(h, who, &rec, false, n_steps, n, A.per_col))
      return rc;
    if (const int rc = slod_lod_source_check(h, who, src, n_steps + 1, "n_steps + 1", n, A.per_col))
      return rc;
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape w = lod_shape(h, n);
    const size_t   nmat = solve.cg() ? (size_t)w.NP * w.cap * w.s * w.s : 0, nvec = (size_t)w.nrow * n;
    // one allocation for the whole loop: S (CG), g, delta, the workspace of the solve and, driven by a source, two loads
    double    *S, *g, *delta, *lb;
    hipError_t e = solve.alloc(n, [&](SlodCarver &c) {
      S = c.take(nmat), g = c.take(nvec), delta = c.take(nvec), solve.take(c, h), lb = c.take(src.armed ? 2 * nvec : 0);
    });
    if (e == hipSuccess)
      {
        if (solve.cg())
          {
            slod_lod_combine_launch(st, nmat, 1.0, d_mass, theta * dt, A.values, S);
            solve.S = S;
            e       = hipGetLastError();
          }
        if (rec.armed)
          slod_lod_record_launch(st, rec, 0, n, A.per_col, d_u, ld_u, nullptr, 0);
        for (int k = 0; k < n_steps && e == hipSuccess; ++k)
          {
            const double *b0 = d_load ? d_load + (size_t)k * load_step_stride : nullptr;
            const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
            size_t        ld_b = ld_load;
            if (src.armed) // b^k and b^(k+1) = the loads + O^T g of the samples k and k + 1, in one launch
              {
                slod_lod_source_launch(st, src, k, 2, n, A.per_col, b0, ld_load, load_step_stride, lb, nvec);
                b0 = lb, b1 = lb + nvec, ld_b = (size_t)n;
              }
            slod_lod_apply_launch(h, st, A, d_cols, d_u, ld_u, n, g, (size_t)n);
            hipLaunchKernelGGL(k_theta_rhs, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n, dt, theta, b0, b1, ld_b, g);
            e = hipGetLastError();
            if (e == hipSuccess)
              e = solve.solve(h, st, k, n, g, (size_t)n, delta, (size_t)n);
            if (e != hipSuccess)
              break;
            hipLaunchKernelGGL(k_theta_advance, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n, delta, d_u, ld_u);
            if (const int j = rec.slot(k + 1); j >= 0)
              slod_lod_record_launch(st, rec, j, n, A.per_col, d_u, ld_u, nullptr, 0);
            e = hipGetLastError();
          }
        // on every path, a failed one too: the workspace is freed on return and a queued kernel may still touch it
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess)
          e = es;
      }
    return e == hipSuccess ? solve.work.worst : slod_hip_fail(h, e, who);
  }
} // namespace

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
  return theta_steps(h, "slod_lod_theta_steps", {SLOD_SOLVE_CG, nullptr, d_cols, nullptr, rel_tol, max_iterations, iterations, rel_residual},
                     {d_stiffness}, d_mass, d_cols, dt, theta, n_steps, n_rhs, d_u, ld_u, d_load, ld_load, load_step_stride);
}

// slod_lod_theta_steps with the factor's two sweeps in place of the CG recurrence
int slod_lod_theta_steps_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const uint32_t *d_cols, double dt,
                                double theta, int n_steps, int n_rhs, double *d_u, size_t ld_u, const double *d_load, size_t ld_load,
                                size_t load_step_stride)
{
  return theta_steps(h, "slod_lod_theta_steps_direct", {SLOD_SOLVE_FACTOR, f_S}, {d_stiffness}, nullptr, d_cols, dt, theta, n_steps,
                     n_rhs, d_u, ld_u, d_load, ld_load, load_step_stride);
}

// slod_lod_theta_steps_direct with a matrix and a factor per column: the product is k_ens_apply (slod_lod_ensemble.hip),
// the solve the member axis of k_factor_solve with one column per member; k_theta_rhs and k_theta_advance work per
// (row, column) and serve as they are.
int slod_lod_theta_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_m,
                                         const uint32_t *d_cols, double dt, double theta, int n_steps, int n_members, double *d_u,
                                         size_t ld_u, const double *d_load, size_t ld_load, size_t load_step_stride)
{
  return theta_steps(h, "slod_lod_theta_steps_ensemble_direct", {SLOD_SOLVE_FACTOR_PER_COL, f_S}, {d_stiffness, ld_m, true}, nullptr,
                     d_cols, dt, theta, n_steps, n_members, d_u, ld_u, d_load, ld_load, load_step_stride);
}

} // extern "C"
#pragma GCC visibility pop
