// Second-order time stepping on the LOD space,  M u'' + C u' + A u = b(t)  with Rayleigh damping
// C = damp_mass M + damp_stiff A  (the reference has no counterpart: it solves one stationary problem,
// LOD.cc:976-1002):
//   slod_lod_inner_multi    out[c] = x_c^T (A y_c), the energies of the stepper
//   slod_lod_newmark_accel  M a = b^0 - A (u + damp_stiff v) - damp_mass M v, the consistent initial acceleration
//   slod_lod_newmark_steps  n_steps of Newmark-beta in acceleration form, the state stays on the device
// and, on a factor the caller built (slod_lod_factor.hip), the _direct calls and their _ensemble_direct forms with a
// matrix, a factor and a column per member: there k_lod_inner and k_nm_rhs run with PER_COL set, the same chains and sums
// on member k's words of a member-minor ensemble matrix (include/slod.h), so column k keeps the bits of the single call.
// The solves are the recurrence of slod_lod_solve_multi (SlodLodWork::solve, slod_lod_multi.hip) on a workspace this
// file owns for the whole loop, every one from zero; row products, tiling and sums are those of slod_lod_tile.hip.h.
// Everything else is elementwise with fp contract off, so the bits of a column depend on that column alone.
#include "slod_lod_tile.hip.h"

#include <algorithm>
#include <vector>

namespace
{
  constexpr int INNER_MAX_BLOCKS = 256; // blocks per chunk

  // one bilinear form x^T (A y) per blockIdx.z; partial: [ngroup][n_rhs]; ld_m: of an ensemble matrix (PER_COL)
  struct InnerJob
  {
    const double *values, *x, *y;
    size_t        ld_x, ld_y;
    double       *partial;
    size_t        ld_m = 1;
  };

  // partial[g][col] = sum over the rows i of group g, ascending, of  x[i,col] * (A y)[i,col].  (A y)[i,col] is the fma
  // chain of k_lod_apply, the product with x is rounded on its own.  PER_COL: column col reads member col of the job's
  // ensemble matrix (the chain of k_ens_apply); the two jobs may differ in ld_m.
  template <bool PER_COL>
  __global__ __launch_bounds__(LOD_BLOCK) void k_lod_inner(int nrow, int s, int cap, int NP, int n_rhs, int ngroup,
                                                         const uint32_t *__restrict__ cols, InnerJob j0, InnerJob j1)
  {
#pragma clang fp contract(off)
    __shared__ double buf[LOD_ROWS][LOD_COLS];
    const InnerJob    J = blockIdx.z ? j1 : j0;
    const int         c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_rhs - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    prod = 0.0;
            if (i < nrow)
              {
                const double acc = slod_lod_row_product<PER_COL>(i, s, cap, NP, J.values, cols, J.y, J.ld_y, col, J.ld_m);
                prod             = J.x[(size_t)i * J.ld_x + col] * acc;
              }
            buf[lr][c] = prod;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb)
          J.partial[(size_t)g * n_rhs + c0 + threadIdx.x] = slod_lod_group_sum(buf, threadIdx.x);
        __syncthreads();
      }
  }

  // out[z][col] = scale * sum of partial_z[g][col], g ascending: one thread per (form z, column)
  __global__ __launch_bounds__(LOD_BLOCK) void k_lod_inner_sum(int n_rhs, int ngroup, int nform, const double *p0, const double *p1,
                                                             double scale, double *out)
  {
#pragma clang fp contract(off)
    const int w = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (w >= nform * n_rhs)
      return;
    const int z = w / n_rhs, col = w - z * n_rhs;
    out[w]      = scale * slod_lod_ordered_sum(z ? p1 : p0, ngroup, n_rhs, col);
  }

  // w = u + damp_stiff v, the argument of A in the right-hand side of the initial acceleration
  __global__ __launch_bounds__(256) void k_nm_shift(int nrow, int n_rhs, double damp_stiff, const double *u, size_t ld_u,
                                                   const double *v, size_t ld_v, double *w)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const size_t i = t / n_rhs, c = t - i * n_rhs;
    const double dv = damp_stiff * v[i * ld_v + c];
    w[t]            = u[i * ld_u + c] + dv;
  }

  // predictor in place,  u~ = u + dt v + dt^2 (1/2 - beta) a,  v~ = v + dt (1 - gamma) a,  and  w = u~ + damp_stiff v~
  // (cv = dt, ca = dt^2 (1/2 - beta), cg = dt (1 - gamma))
  __global__ __launch_bounds__(256) void k_nm_predict(int nrow, int n_rhs, double cv, double ca, double cg, double damp_stiff, double *u,
                                                     size_t ld_u, double *v, size_t ld_v, const double *a, size_t ld_a, double *w)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const size_t i = t / n_rhs, c = t - i * n_rhs;
    const double ui = u[i * ld_u + c], vi = v[i * ld_v + c], ai = a[i * ld_a + c];
    const double tv = cv * vi, ta = ca * ai, tg = cg * ai;
    const double up = (ui + tv) + ta, vp = vi + tg;
    const double dv = damp_stiff * vp;
    u[i * ld_u + c] = up;
    v[i * ld_v + c] = vp;
    w[t]            = up + dv;
  }

  // g = (b - A w) - damp_mass (M v) per (row, column); load NULL: b = 0; mass NULL: no mass term (damp_mass = 0).
  // PER_COL: column c reads member c of the ensemble matrices stiffness (ld_a_m) and mass (ld_m_m).
  template <bool PER_COL>
  __global__ __launch_bounds__(256) void k_nm_rhs(int nrow, int s, int cap, int NP, int n_rhs, const double *__restrict__ stiffness,
                                                 size_t ld_a_m, const double *__restrict__ mass, size_t ld_m_m,
                                                 const uint32_t *__restrict__ cols, double damp_mass, const double *load,
                                                 size_t ld_load, const double *w, const double *v, size_t ld_v, double *g)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const int    i = (int)(t / n_rhs), c = (int)(t - (size_t)i * n_rhs);
    const double Aw = slod_lod_row_product<PER_COL>(i, s, cap, NP, stiffness, cols, w, (size_t)n_rhs, c, ld_a_m);
    double       r = (load ? load[(size_t)i * ld_load + c] : 0.0) - Aw;
    if (mass)
      {
        const double Mv = slod_lod_row_product<PER_COL>(i, s, cap, NP, mass, cols, v, ld_v, c, ld_m_m);
        const double dm = damp_mass * Mv;
        r               = r - dm;
      }
    g[t] = r;
  }

  // corrector in place,  u = u~ + beta dt^2 a,  v = v~ + gamma dt a  (cu = beta dt^2, cv = gamma dt)
  __global__ __launch_bounds__(256) void k_nm_correct(int nrow, int n_rhs, double cu, double cv, double *u, size_t ld_u, double *v,
                                                     size_t ld_v, const double *a, size_t ld_a)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const size_t i = t / n_rhs, c = t - i * n_rhs;
    const double ai = a[i * ld_a + c];
    const double tu = cu * ai, tv = cv * ai;
    u[i * ld_u + c] = u[i * ld_u + c] + tu;
    v[i * ld_v + c] = v[i * ld_v + c] + tv;
  }

  // The matrices of a time loop: one pair for all columns, or (per_col) a member per column of two ensemble matrices
  struct NmMatrices
  {
    const double *stiffness, *mass;
    size_t        ld_a_m = 1, ld_m_m = 1;
    bool          per_col = false;
  };

  // nform (1 or 2) bilinear forms in one launch of k_lod_inner, then their ordered sums: out[z * n_rhs + col]
  void launch_inner(const LodShape &w, hipStream_t st, const uint32_t *cols, int n_rhs, int nform, const InnerJob &j0,
                    const InnerJob &j1, double scale, double *out, bool per_col = false)
  {
    hipLaunchKernelGGL(per_col ? k_lod_inner<true> : k_lod_inner<false>, lod_grid(w, INNER_MAX_BLOCKS, nform), dim3(LOD_BLOCK), 0, st,
                       w.nrow, w.s, w.cap, w.NP, n_rhs, w.ngroup, cols, j0, j1);
    hipLaunchKernelGGL(k_lod_inner_sum, lod_flat_grid((size_t)nform * n_rhs), dim3(LOD_BLOCK), 0, st, n_rhs, w.ngroup, nform,
                       j0.partial, j1.partial, scale, out);
  }

  // g = (b - A arg) - damp_mass (M v) on n_rhs columns; the mass product is skipped when damp_mass = 0
  void launch_rhs(const LodShape &w, hipStream_t st, const NmMatrices &m, const uint32_t *cols, int n_rhs, double damp_mass,
                  const double *load, size_t ld_load, const double *arg, const double *v, size_t ld_v, double *g)
  {
    hipLaunchKernelGGL(m.per_col ? k_nm_rhs<true> : k_nm_rhs<false>, lod_flat_grid((size_t)w.nrow * n_rhs), dim3(256), 0, st, w.nrow,
                       w.s, w.cap, w.NP, n_rhs, m.stiffness, m.ld_a_m, damp_mass != 0.0 ? m.mass : nullptr, m.ld_m_m, cols, damp_mass,
                       load, ld_load, arg, v, ld_v, g);
  }

  bool bad_damping(double damp_mass, double damp_stiff) { return !(damp_mass >= 0.0) || !(damp_stiff >= 0.0); }

  // The device work of slod_lod_newmark_accel_direct and of its ensemble form (m.per_col: column k on member k of f_M);
  // arguments are checked by the caller
  int nm_accel_direct(slod_handle *h, const char *who, slod_lod_factor *f_M, const NmMatrices &m, const uint32_t *d_cols,
                      double damp_mass, double damp_stiff, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                      const double *d_load, size_t ld_load, double *d_a, size_t ld_a)
  {
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape     w = lod_shape(h, n_rhs);
    const size_t       nvec = (size_t)w.nrow * n_rhs;
    SlodDevBuf<double> work; // w = u + damp_stiff v, g
    hipError_t         e = work.alloc(2 * nvec);
    if (e == hipSuccess)
      {
        double *arg = work.get(), *g = arg + nvec;
        hipLaunchKernelGGL(k_nm_shift, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_rhs, damp_stiff, d_u, ld_u, d_v, ld_v, arg);
        launch_rhs(w, st, m, d_cols, n_rhs, damp_mass, d_load, ld_load, arg, d_v, ld_v, g);
        if (m.per_col)
          slod_lod_factor_solve_launch(f_M, st, g, (size_t)n_rhs, 1, d_a, ld_a, 0, n_rhs);
        else
          slod_lod_factor_solve_launch(f_M, st, g, (size_t)n_rhs, n_rhs, d_a, ld_a);
        e = hipGetLastError();
        const hipError_t es = hipStreamSynchronize(st); // the workspace is freed on return
        if (e == hipSuccess)
          e = es;
      }
    return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
  }

  // The device work of slod_lod_newmark_steps_direct and of its ensemble form: the whole loop is queued and the stream is
  // waited for once; arguments are checked by the caller
  int nm_steps_direct(slod_handle *h, const char *who, slod_lod_factor *f_S, const NmMatrices &m, const uint32_t *d_cols, double dt,
                      double beta, double gamma, double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                      double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load, size_t ld_load,
                      size_t load_step_stride, double *kinetic, double *potential)
  {
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape w = lod_shape(h, n_rhs);
    const bool     energies = kinetic != nullptr;
    const size_t   nvec = (size_t)w.nrow * n_rhs, npart = energies ? (size_t)w.ngroup * n_rhs : 0;
    const size_t   nenergy = energies ? 2 * (size_t)(n_steps + 1) * n_rhs : 0;
    // w = u~ + damp_stiff v~, g, and for the energies two arrays of partials and [level][kinetic, potential][column]
    SlodDevBuf<double> work;
    hipError_t         e = work.alloc(2 * nvec + 2 * npart + nenergy);
    if (e == hipSuccess)
      {
        double        *arg = work.get(), *g = arg + nvec, *part_k = g + nvec, *part_p = part_k + npart, *d_energy = part_p + npart;
        const dim3     nblk = lod_flat_grid(nvec);
        const InnerJob jk{m.mass, d_v, d_v, ld_v, ld_v, part_k, m.ld_m_m}, jp{m.stiffness, d_u, d_u, ld_u, ld_u, part_p, m.ld_a_m};
        const double   gdt = gamma * dt, bdt2 = beta * dt * dt;
        if (energies)
          launch_inner(w, st, d_cols, n_rhs, 2, jk, jp, 0.5, d_energy, m.per_col);
        e = hipGetLastError();
        for (int k = 0; k < n_steps && e == hipSuccess; ++k)
          {
            const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
            hipLaunchKernelGGL(k_nm_predict, nblk, dim3(256), 0, st, w.nrow, n_rhs, dt, dt * dt * (0.5 - beta), dt * (1.0 - gamma),
                               damp_stiff, d_u, ld_u, d_v, ld_v, d_a, ld_a, arg);
            launch_rhs(w, st, m, d_cols, n_rhs, damp_mass, b1, ld_load, arg, d_v, ld_v, g);
            if (m.per_col)
              slod_lod_factor_solve_launch(f_S, st, g, (size_t)n_rhs, 1, d_a, ld_a, 0, n_rhs);
            else
              slod_lod_factor_solve_launch(f_S, st, g, (size_t)n_rhs, n_rhs, d_a, ld_a);
            hipLaunchKernelGGL(k_nm_correct, nblk, dim3(256), 0, st, w.nrow, n_rhs, bdt2, gdt, d_u, ld_u, d_v, ld_v, d_a, ld_a);
            if (energies)
              launch_inner(w, st, d_cols, n_rhs, 2, jk, jp, 0.5, d_energy + 2 * (size_t)(k + 1) * n_rhs, m.per_col);
            e = hipGetLastError();
          }
        std::vector<double> host(nenergy);
        if (e == hipSuccess && energies)
          e = hipMemcpyAsync(host.data(), d_energy, nenergy * sizeof(double), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st); // the workspace is freed on return
        if (e == hipSuccess)
          e = es;
        if (e == hipSuccess && energies)
          for (size_t k = 0; k <= (size_t)n_steps; ++k)
            for (size_t c = 0; c < (size_t)n_rhs; ++c)
              {
                kinetic[k * n_rhs + c]   = host[2 * k * n_rhs + c];
                potential[k * n_rhs + c] = host[(2 * k + 1) * n_rhs + c];
              }
      }
    return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
  }

  // The checks the two ensemble steppers share, in the order of the single calls
  int nm_ensemble_check(const slod_handle *h, const std::string &who, bool arrays, double damp_mass, double damp_stiff, int n_members,
                        std::initializer_list<size_t> lds)
  {
    if (!h || !arrays)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL handle, matrix, d_cols or state");
    if (bad_damping(damp_mass, damp_stiff))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": negative or NaN damping coefficient");
    if (n_members < 1 || n_members > 65535)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_members < 1 or > 65535");
    return slod_check_ld(h, who.c_str(), "n_members", n_members, lds);
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_inner_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                         const double *d_y, size_t ld_y, int n_rhs, double *out, void *hip_stream)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_values || !d_cols || !d_x || !d_y || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_inner_multi: NULL array");
  if (n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_inner_multi: n_rhs < 1");
  if (const int rc = slod_check_ld(h, "slod_lod_inner_multi", "n_rhs", n_rhs, {ld_x, ld_y}))
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const LodShape     w = lod_shape(h, n_rhs);
  SlodDevBuf<double> work; // the partials, then the n_rhs sums
  hipError_t         e = work.alloc((size_t)w.ngroup * n_rhs + (size_t)n_rhs);
  if (e == hipSuccess)
    {
      const InnerJob job{d_values, d_x, d_y, ld_x, ld_y, work.get()};
      double        *d_out = work.get() + (size_t)w.ngroup * n_rhs;
      launch_inner(w, st, d_cols, n_rhs, 1, job, job, 1.0, d_out);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(out, d_out, (size_t)n_rhs * sizeof(double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess)
        e = hipStreamSynchronize(st); // work is freed on return
    }
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_inner_multi");
}

int slod_lod_newmark_accel(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double damp_mass,
                           double damp_stiff, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                           const double *d_load, size_t ld_load, double *d_a, size_t ld_a, double rel_tol, int max_iterations,
                           int *iterations, double *rel_residual)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_stiffness || !d_mass || !d_cols || !d_u || !d_v || !d_a)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_accel: NULL matrix, d_cols or state");
  if (bad_damping(damp_mass, damp_stiff))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_accel: negative or NaN damping coefficient");
  if (n_rhs < 1 || max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_accel: n_rhs < 1 or max_iterations < 0");
  if (const int rc = slod_check_ld(h, "slod_lod_newmark_accel", "n_rhs", n_rhs, {ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}))
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const LodShape w = lod_shape(h, n_rhs);
  const size_t   nvec = (size_t)w.nrow * n_rhs;
  // w = u + damp_stiff v, g, and the workspace of the solve
  double     *arg, *g;
  SlodLodWork work;
  hipError_t  e = work.alloc(n_rhs, [&](SlodCarver &c) { arg = c.take(nvec), g = c.take(nvec), work.take_solve(c, h); });
  if (e == hipSuccess)
    {
      hipLaunchKernelGGL(k_nm_shift, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n_rhs, damp_stiff, d_u, ld_u, d_v, ld_v, arg);
      launch_rhs(w, st, {d_stiffness, d_mass}, d_cols, n_rhs, damp_mass, d_load, ld_load, arg, d_v, ld_v, g);
      e = hipGetLastError();
      if (e == hipSuccess) // the solve synchronises: the workspace is freed on return
        e = work.solve(h, d_mass, d_cols, g, (size_t)n_rhs, d_a, ld_a, rel_tol, max_iterations);
    }
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_lod_newmark_accel");
  work.report(iterations, rel_residual);
  return work.last;
}

int slod_lod_newmark_steps(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double dt,
                           double beta, double gamma, double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u,
                           size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load, size_t ld_load,
                           size_t load_step_stride, double rel_tol, int max_iterations, int *iterations, double *rel_residual,
                           double *kinetic, double *potential)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_stiffness || !d_mass || !d_cols || !d_u || !d_v || !d_a)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps: NULL matrix, d_cols or state");
  if (!(dt > 0.0) || !(beta >= 0.0 && beta <= 0.5) || !(gamma >= 0.0 && gamma <= 1.0))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]");
  if (bad_damping(damp_mass, damp_stiff))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps: negative or NaN damping coefficient");
  if (n_steps < 1 || n_rhs < 1 || max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0");
  if (const int rc = slod_check_ld(h, "slod_lod_newmark_steps", "n_rhs", n_rhs, {ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}))
    return rc;
  if ((kinetic == nullptr) != (potential == nullptr))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps: kinetic and potential come together or not at all");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const LodShape w = lod_shape(h, n_rhs);
  const bool     energies = kinetic != nullptr;
  const size_t   nmat = (size_t)w.NP * w.cap * w.s * w.s, nvec = (size_t)w.nrow * n_rhs, npart = (size_t)w.ngroup * n_rhs;
  const size_t   nenergy = energies ? 2 * (size_t)(n_steps + 1) * n_rhs : 0;
  // one allocation for the whole loop: S, w = u~ + damp_stiff v~, g, the workspace of the solve, and for the
  // energies two arrays of partials and [level][kinetic, potential][column]
  double     *S, *arg, *g, *part_k, *part_p, *d_energy;
  SlodLodWork work;
  hipError_t  e = work.alloc(n_rhs, [&](SlodCarver &c) {
    S = c.take(nmat), arg = c.take(nvec), g = c.take(nvec), work.take_solve(c, h);
    part_k = c.take(energies ? npart : 0), part_p = c.take(energies ? npart : 0), d_energy = c.take(nenergy);
  });
  if (e == hipSuccess)
    {
      const dim3     nblk = lod_flat_grid(nvec);
      const InnerJob jk{d_mass, d_v, d_v, ld_v, ld_v, part_k}, jp{d_stiffness, d_u, d_u, ld_u, ld_u, part_p};
      const double   gdt = gamma * dt, bdt2 = beta * dt * dt;
      slod_lod_combine_launch(st, nmat, 1.0 + gdt * damp_mass, d_mass, bdt2 + gdt * damp_stiff, d_stiffness, S);
      if (energies)
        launch_inner(w, st, d_cols, n_rhs, 2, jk, jp, 0.5, d_energy);
      e = hipGetLastError();
      for (int k = 0; k < n_steps && e == hipSuccess; ++k)
        {
          const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
          hipLaunchKernelGGL(k_nm_predict, nblk, dim3(256), 0, st, w.nrow, n_rhs, dt, dt * dt * (0.5 - beta), dt * (1.0 - gamma),
                             damp_stiff, d_u, ld_u, d_v, ld_v, d_a, ld_a, arg);
          launch_rhs(w, st, {d_stiffness, d_mass}, d_cols, n_rhs, damp_mass, b1, ld_load, arg, d_v, ld_v, g);
          e = hipGetLastError();
          if (e == hipSuccess)
            e = work.solve(h, S, d_cols, g, (size_t)n_rhs, d_a, ld_a, rel_tol, max_iterations);
          if (e != hipSuccess)
            break;
          work.record(k, iterations, rel_residual);
          hipLaunchKernelGGL(k_nm_correct, nblk, dim3(256), 0, st, w.nrow, n_rhs, bdt2, gdt, d_u, ld_u, d_v, ld_v, d_a, ld_a);
          if (energies)
            launch_inner(w, st, d_cols, n_rhs, 2, jk, jp, 0.5, d_energy + 2 * (size_t)(k + 1) * n_rhs);
          e = hipGetLastError();
        }
      std::vector<double> host(nenergy);
      if (e == hipSuccess && energies)
        e = hipMemcpyAsync(host.data(), d_energy, nenergy * sizeof(double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess)
        e = hipStreamSynchronize(st); // the workspace is freed on return
      if (e == hipSuccess && energies)
        for (size_t k = 0; k <= (size_t)n_steps; ++k)
          for (size_t c = 0; c < (size_t)n_rhs; ++c)
            {
              kinetic[k * n_rhs + c]   = host[2 * k * n_rhs + c];
              potential[k * n_rhs + c] = host[(2 * k + 1) * n_rhs + c];
            }
    }
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_lod_newmark_steps");
  return work.worst;
}

// slod_lod_newmark_accel with the factor of M in place of the CG recurrence
int slod_lod_newmark_accel_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, const double *d_mass,
                                  const uint32_t *d_cols, double damp_mass, double damp_stiff, int n_rhs, const double *d_u, size_t ld_u,
                                  const double *d_v, size_t ld_v, const double *d_load, size_t ld_load, double *d_a, size_t ld_a)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_stiffness || !d_mass || !d_cols || !d_u || !d_v || !d_a)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_accel_direct: NULL matrix, d_cols or state");
  if (bad_damping(damp_mass, damp_stiff))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_accel_direct: negative or NaN damping coefficient");
  if (n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_accel_direct: n_rhs < 1");
  if (const int rc = slod_check_ld(h, "slod_lod_newmark_accel_direct", "n_rhs", n_rhs, {ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}))
    return rc;
  if (const int rc = slod_lod_factor_check(h, "slod_lod_newmark_accel_direct", f_M)) // last: it reads the factor
    return rc;
  return nm_accel_direct(h, "slod_lod_newmark_accel_direct", f_M, {d_stiffness, d_mass}, d_cols, damp_mass, damp_stiff, n_rhs, d_u, ld_u,
                         d_v, ld_v, d_load, ld_load, d_a, ld_a);
}

// The loop of slod_lod_newmark_steps with the factor's two sweeps in place of the CG recurrence
int slod_lod_newmark_steps_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const double *d_mass,
                                  const uint32_t *d_cols, double dt, double beta, double gamma, double damp_mass, double damp_stiff,
                                  int n_steps, int n_rhs, double *d_u, size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a,
                                  const double *d_load, size_t ld_load, size_t load_step_stride, double *kinetic, double *potential)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_stiffness || !d_mass || !d_cols || !d_u || !d_v || !d_a)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps_direct: NULL matrix, d_cols or state");
  if (!(dt > 0.0) || !(beta >= 0.0 && beta <= 0.5) || !(gamma >= 0.0 && gamma <= 1.0))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]");
  if (bad_damping(damp_mass, damp_stiff))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps_direct: negative or NaN damping coefficient");
  if (n_steps < 1 || n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps_direct: n_steps < 1 or n_rhs < 1");
  if (const int rc = slod_check_ld(h, "slod_lod_newmark_steps_direct", "n_rhs", n_rhs, {ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}))
    return rc;
  if ((kinetic == nullptr) != (potential == nullptr))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_newmark_steps_direct: kinetic and potential come together or not at all");
  if (const int rc = slod_lod_factor_check(h, "slod_lod_newmark_steps_direct", f_S)) // last: it reads the factor
    return rc;
  return nm_steps_direct(h, "slod_lod_newmark_steps_direct", f_S, {d_stiffness, d_mass}, d_cols, dt, beta, gamma, damp_mass, damp_stiff,
                         n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_a, ld_a, d_load, ld_load, load_step_stride, kinetic, potential);
}

// slod_lod_inner_multi with a matrix per column: k_lod_inner<true>, then the same ordered sums
int slod_lod_inner_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                            const double *d_y, size_t ld_y, int n_members, double *out, void *hip_stream)
{
  const std::string who = "slod_lod_inner_ensemble";
  if (!h || !d_values || !d_cols || !d_x || !d_y || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL handle or array");
  if (n_members < 1 || n_members > 65535)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_members < 1 or > 65535");
  if (const int rc = slod_check_ld(h, who.c_str(), "n_members", n_members, {ld_m, ld_x, ld_y}))
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const LodShape     w = lod_shape(h, n_members);
  SlodDevBuf<double> work; // the partials, then the n_members sums
  hipError_t         e = work.alloc((size_t)w.ngroup * n_members + (size_t)n_members);
  if (e == hipSuccess)
    {
      const InnerJob job{d_values, d_x, d_y, ld_x, ld_y, work.get(), ld_m};
      double        *d_out = work.get() + (size_t)w.ngroup * n_members;
      launch_inner(w, st, d_cols, n_members, 1, job, job, 1.0, d_out, true);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(out, d_out, (size_t)n_members * sizeof(double), hipMemcpyDeviceToHost, st);
      const hipError_t es = hipStreamSynchronize(st); // work is freed on return
      if (e == hipSuccess)
        e = es;
    }
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who.c_str());
}

// slod_lod_newmark_accel_direct with a matrix, a factor and a column per member
int slod_lod_newmark_accel_ensemble_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, size_t ld_a_m,
                                           const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, double damp_mass,
                                           double damp_stiff, int n_members, const double *d_u, size_t ld_u, const double *d_v,
                                           size_t ld_v, const double *d_load, size_t ld_load, double *d_a, size_t ld_a)
{
  const char *who = "slod_lod_newmark_accel_ensemble_direct";
  if (const int rc = nm_ensemble_check(h, who, d_stiffness && d_mass && d_cols && d_u && d_v && d_a, damp_mass, damp_stiff, n_members,
                                       {ld_a_m, ld_m_m, ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}))
    return rc;
  if (const int rc = slod_lod_factor_check(h, who, f_M, n_members)) // last: it reads the factor
    return rc;
  return nm_accel_direct(h, who, f_M, {d_stiffness, d_mass, ld_a_m, ld_m_m, true}, d_cols, damp_mass, damp_stiff, n_members, d_u, ld_u,
                         d_v, ld_v, d_load, ld_load, d_a, ld_a);
}

// The loop of slod_lod_newmark_steps_direct with a matrix, a factor and a column per member
int slod_lod_newmark_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_a_m,
                                           const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, double dt, double beta,
                                           double gamma, double damp_mass, double damp_stiff, int n_steps, int n_members, double *d_u,
                                           size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load,
                                           size_t ld_load, size_t load_step_stride, double *kinetic, double *potential)
{
  const std::string who = "slod_lod_newmark_steps_ensemble_direct";
  if (!h || !d_stiffness || !d_mass || !d_cols || !d_u || !d_v || !d_a)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL handle, matrix, d_cols or state");
  if (!(dt > 0.0) || !(beta >= 0.0 && beta <= 0.5) || !(gamma >= 0.0 && gamma <= 1.0))
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]");
  if (n_steps < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_steps < 1");
  if (const int rc = nm_ensemble_check(h, who, true, damp_mass, damp_stiff, n_members,
                                       {ld_a_m, ld_m_m, ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}))
    return rc;
  if ((kinetic == nullptr) != (potential == nullptr))
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": kinetic and potential come together or not at all");
  if (const int rc = slod_lod_factor_check(h, who.c_str(), f_S, n_members)) // last: it reads the factor
    return rc;
  return nm_steps_direct(h, who.c_str(), f_S, {d_stiffness, d_mass, ld_a_m, ld_m_m, true}, d_cols, dt, beta, gamma, damp_mass,
                         damp_stiff, n_steps, n_members, d_u, ld_u, d_v, ld_v, d_a, ld_a, d_load, ld_load, load_step_stride, kinetic,
                         potential);
}

} // extern "C"
#pragma GCC visibility pop
