// Second-order time stepping on the LOD space,  M u'' + C u' + A u = b(t)  with Rayleigh damping
// C = damp_mass M + damp_stiff A  (the reference has no counterpart: it solves one stationary problem,
// LOD.cc:976-1002):
//   slod_lod_inner_multi    out[c] = x_c^T (A y_c), the energies of the stepper
//   slod_lod_newmark_accel  M a = b^0 - A (u + damp_stiff v) - damp_mass M v, the consistent initial acceleration
//   slod_lod_newmark_steps  n_steps of Newmark-beta in acceleration form, the state stays on the device
// and, on a factor the caller built (slod_lod_factor.hip), the _direct calls and their _ensemble_direct forms with a
// matrix, a factor and a column per member: there k_lod_inner and k_nm_rhs run with PER_COL set, the same chains and sums
// on member k's words of a member-minor ensemble matrix (include/slod.h), so column k keeps the bits of the single call.
// Each scheme is written once on the operator of a column and the solve of a step (SlodLodOperator, SlodLodStepSolve,
// slod_host.h): inner, nm_accel and nm_steps serve the CG call, the _direct call and the _ensemble_direct call, and
// inner_check / nm_check hold their argument checks, every call with its own wording.  The CG solves are the recurrence
// of slod_lod_solve_multi (SlodLodWork::solve, slod_lod_multi.hip) on a workspace the loop owns, every one from zero; on
// a factor the whole loop is queued and waited for once.  Row products, tiling and sums are those of slod_lod_tile.hip.h.
// Everything else is elementwise with fp contract off, so the bits of a column depend on that column alone.
// The _damped calls add a third matrix to the damping, C = damp_mass M + damp_stiff A + D (a sponge layer: D = C^T M_sigma C
// of slod_lod_mass_matrix with d_rho = sigma): the bodies take it as an optional third operator, k_nm_rhs<.., true> forms
// M v and D v in one walk over the row, and a call without D runs the launches and has the words it had before.
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

  // (M x)_i and (D x)_i of row i in one walk over its slots: the column indices and x are read once, every chain is the
  // fma chain of slod_lod_row_product on its own operands.  HAS_M unset: the D chain alone (accm stays 0).
  template <bool HAS_M>
  __device__ __forceinline__ void nm_damping_products(int i, int s, int cap, int NP, const double *__restrict__ m,
                                                      const double *__restrict__ dmat, const uint32_t *__restrict__ cols,
                                                      const double *__restrict__ x, size_t ld, int col, double &accm, double &accd)
  {
    const int    p = i / s, d = i - p * s;
    const size_t slot0 = (size_t)p * cap;
    accm = accd = 0.0;
    for (int j = 0; j < cap; ++j)
      {
        const uint32_t q = cols[slot0 + j];
        const bool     used = q < (uint32_t)NP;
        const size_t   qs = (size_t)(used ? q : (uint32_t)p) * s, at = (slot0 + j) * s * s + d * s;
        for (int e = 0; e < s; ++e)
          {
            const double xv = x[(qs + e) * ld + col];
            const double td = fma(dmat[at + e], xv, accd);
            accd            = used ? td : accd;
            if constexpr (HAS_M)
              {
                const double tm = fma(m[at + e], xv, accm);
                accm            = used ? tm : accm;
              }
          }
      }
  }

  // g = (b - A w) - damp_mass (M v) per (row, column); load NULL: b = 0; mass NULL: no mass term (damp_mass = 0).
  // PER_COL: column c reads member c of the ensemble matrices stiffness (ld_a_m) and mass (ld_m_m).
  // DAMPED: g = ((b - A w) - damp_mass (M v)) - (D v) with the third matrix damping (ld_d_m); M v and D v come from one
  // walk over the row (with a member per column: from a product each).
  template <bool PER_COL, bool DAMPED = false>
  __global__ __launch_bounds__(256) void k_nm_rhs(int nrow, int s, int cap, int NP, int n_rhs, const double *__restrict__ stiffness,
                                                 size_t ld_a_m, const double *__restrict__ mass, size_t ld_m_m,
                                                 const double *__restrict__ damping, size_t ld_d_m,
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
    if constexpr (DAMPED)
      {
        double Mv = 0.0, Dv;
        if constexpr (PER_COL)
          {
            if (mass)
              Mv = slod_lod_row_product<true>(i, s, cap, NP, mass, cols, v, ld_v, c, ld_m_m);
            Dv = slod_lod_row_product<true>(i, s, cap, NP, damping, cols, v, ld_v, c, ld_d_m);
          }
        else if (mass)
          nm_damping_products<true>(i, s, cap, NP, mass, damping, cols, v, ld_v, c, Mv, Dv);
        else
          nm_damping_products<false>(i, s, cap, NP, nullptr, damping, cols, v, ld_v, c, Mv, Dv);
        if (mass)
          {
            const double dm = damp_mass * Mv;
            r               = r - dm;
          }
        r = r - Dv;
      }
    else if (mass)
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

  // the form x^T (A y) of a job: its matrix is the operator's, one for all columns or a member per column
  InnerJob inner_job(const SlodLodOperator &A, const double *x, size_t ld_x, const double *y, size_t ld_y, double *partial)
  {
    return {A.values, x, y, ld_x, ld_y, partial, A.ld_m};
  }

  // nform (1 or 2) bilinear forms in one launch of k_lod_inner, then their ordered sums: out[z * n_rhs + col].  A: the
  // operator of the first job; the second one's has the same per_col.
  void launch_inner(const LodShape &w, hipStream_t st, const SlodLodOperator &A, const uint32_t *cols, int n_rhs, int nform,
                    const InnerJob &j0, const InnerJob &j1, double scale, double *out)
  {
    hipLaunchKernelGGL(A.per_col ? k_lod_inner<true> : k_lod_inner<false>, lod_grid(w, INNER_MAX_BLOCKS, nform), dim3(LOD_BLOCK), 0, st,
                       w.nrow, w.s, w.cap, w.NP, n_rhs, w.ngroup, cols, j0, j1);
    hipLaunchKernelGGL(k_lod_inner_sum, lod_flat_grid((size_t)nform * n_rhs), dim3(LOD_BLOCK), 0, st, n_rhs, w.ngroup, nform,
                       j0.partial, j1.partial, scale, out);
  }

  // g = (b - A arg) - damp_mass (M v) on n_rhs columns; the mass product is skipped when damp_mass = 0.  D.values given:
  // the damped instantiation, g = ((b - A arg) - damp_mass (M v)) - (D v); the ensemble loops pass none.
  void launch_rhs(const LodShape &w, hipStream_t st, const SlodLodOperator &A, const SlodLodOperator &M, const SlodLodOperator &D,
                  const uint32_t *cols, int n_rhs, double damp_mass, const double *load, size_t ld_load, const double *arg,
                  const double *v, size_t ld_v, double *g)
  {
    const auto kernel = D.values ? k_nm_rhs<false, true> : A.per_col ? k_nm_rhs<true> : k_nm_rhs<false>;
    hipLaunchKernelGGL(kernel, lod_flat_grid((size_t)w.nrow * n_rhs), dim3(256), 0, st, w.nrow, w.s, w.cap, w.NP, n_rhs, A.values,
                       A.ld_m, damp_mass != 0.0 ? M.values : nullptr, M.ld_m, D.values, D.ld_m, cols, damp_mass, load, ld_load, arg, v,
                       ld_v, g);
  }

  // out[c] = x_c^T (A y_c) on n columns with the operator of every column: the body of slod_lod_inner_multi and, with a
  // member per column, of slod_lod_inner_ensemble, every call with the wording of its refusals
  int inner(slod_handle *h, const std::string &who, const SlodLodOperator &A, const uint32_t *d_cols, const double *d_x, size_t ld_x,
            const double *d_y, size_t ld_y, int n, double *out, void *hip_stream)
  {
    const bool ens = A.per_col;
    if (!h && !ens)
      return SLOD_ERR_ARGUMENT;
    if (!h || !A.values || !d_cols || !d_x || !d_y || !out)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (ens ? ": NULL handle or array" : ": NULL array"));
    if (n < 1 || (ens && n > 65535))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (ens ? ": n_members < 1 or > 65535" : ": n_rhs < 1"));
    if (const int rc = slod_check_ld_of(h, who.c_str(), ens, {A.ld_m}, n, {ld_x, ld_y}))
      return rc;
    hipStream_t st;
    if (const int rc = slod_enter(h, hip_stream, &st))
      return rc;
    const LodShape     w = lod_shape(h, n);
    SlodDevBuf<double> work; // the partials, then the n sums
    hipError_t         e = work.alloc((size_t)w.ngroup * n + (size_t)n);
    if (e == hipSuccess)
      {
        const InnerJob job = inner_job(A, d_x, ld_x, d_y, ld_y, work.get());
        double        *d_out = work.get() + (size_t)w.ngroup * n;
        launch_inner(w, st, A, d_cols, n, 1, job, job, 1.0, d_out);
        e = hipGetLastError();
        if (e == hipSuccess)
          e = hipMemcpyAsync(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st); // work is freed on return
        if (e == hipSuccess)
          e = es;
      }
    return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who.c_str());
  }

  // The argument checks of the Newmark calls, in one order, every call with its wording.  steps: the checks of the
  // stepper (dt, beta, gamma, n_steps and energy_pair: both energy arrays or neither), else those of the initial
  // acceleration.  state: no vector is NULL; n: n_rhs or n_members; lds: the leading dimensions of the vectors.  The factor
  // is looked at last: only that check reads it.
  int nm_check(const slod_handle *h, const std::string &who, const SlodLodStepSolve &solve, bool steps, const SlodLodOperator &A,
               const SlodLodOperator &M, bool state, double dt, double beta, double gamma, double damp_mass, double damp_stiff,
               int n_steps, int n, std::initializer_list<size_t> lds, bool energy_pair)
  {
    const bool cg = solve.cg(), ens = A.per_col, arrays = A.values && M.values && state;
    const int  max_iterations = solve.max_iterations;
    if (!h && !ens)
      return SLOD_ERR_ARGUMENT;
    if (!h || !arrays)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (ens ? ": NULL handle, matrix, d_cols or state" : ": NULL matrix, d_cols or state"));
    if (steps && (!(dt > 0.0) || !(beta >= 0.0 && beta <= 0.5) || !(gamma >= 0.0 && gamma <= 1.0)))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]");
    if (steps && ens && n_steps < 1) // the ensemble stepper names n_steps on its own, before the damping
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_steps < 1");
    if (!(damp_mass >= 0.0) || !(damp_stiff >= 0.0))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": negative or NaN damping coefficient");
    if (ens && (n < 1 || n > 65535))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_members < 1 or > 65535");
    if (!ens && ((steps && n_steps < 1) || n < 1 || (cg && max_iterations < 0)))
      return slod_fail(h, SLOD_ERR_ARGUMENT,
                       who + (!steps ? ": n_rhs < 1" : cg ? ": n_steps < 1, n_rhs < 1" : ": n_steps < 1 or n_rhs < 1") +
                         (cg ? " or max_iterations < 0" : ""));
    if (const int rc = slod_check_ld_of(h, who.c_str(), ens, {A.ld_m, M.ld_m}, n, lds))
      return rc;
    if (steps && !energy_pair)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": kinetic and potential come together or not at all");
    return cg ? SLOD_OK : slod_lod_factor_check(h, who.c_str(), solve.f, ens ? n : 1);
  }

  // M a = b^0 - A (u + damp_stiff v) - damp_mass M v [- D v] on n columns, whatever solves with M (the CG on M itself, or
  // its factor): the body of the accel calls.  D: the third matrix of the _damped calls, values NULL: none.  iterations, rel_residual: of the CG, per column.  Returns the largest
  // iteration count (0 on a factor) or a negative status.
  int nm_accel(slod_handle *h, const char *who, SlodLodStepSolve &&solve, const SlodLodOperator &A, const SlodLodOperator &M,
               const SlodLodOperator &D, const uint32_t *d_cols, double damp_mass, double damp_stiff, int n, const double *d_u, size_t ld_u, const double *d_v,
               size_t ld_v, const double *d_load, size_t ld_load, double *d_a, size_t ld_a, int *iterations = nullptr,
               double *rel_residual = nullptr)
  {
    if (const int rc = nm_check(h, who, solve, false, A, M, d_cols && d_u && d_v && d_a, 0.0, 0.0, 0.0, damp_mass, damp_stiff, 0, n,
                                {ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}, true))
      return rc;
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape w = lod_shape(h, n);
    const size_t   nvec = (size_t)w.nrow * n;
    // w = u + damp_stiff v, g, and the workspace of the solve
    double    *arg, *g;
    hipError_t e = solve.alloc(n, [&](SlodCarver &c) { arg = c.take(nvec), g = c.take(nvec), solve.take(c, h); });
    if (e == hipSuccess)
      {
        hipLaunchKernelGGL(k_nm_shift, lod_flat_grid(nvec), dim3(256), 0, st, w.nrow, n, damp_stiff, d_u, ld_u, d_v, ld_v, arg);
        launch_rhs(w, st, A, M, D, d_cols, n, damp_mass, d_load, ld_load, arg, d_v, ld_v, g);
        e = hipGetLastError();
        if (e == hipSuccess)
          e = solve.solve(h, st, 0, n, g, (size_t)n, d_a, ld_a);
        if (e == hipSuccess && !solve.cg())
          e = hipGetLastError();
        // the workspace is freed on return; a CG that succeeded has left the stream synchronised
        if (!(solve.cg() && e == hipSuccess))
          {
            const hipError_t es = hipStreamSynchronize(st);
            if (e == hipSuccess)
              e = es;
          }
      }
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who);
    solve.work.report(iterations, rel_residual);
    return solve.work.last;
  }

  // n_steps of Newmark-beta in acceleration form on n columns, whatever solves the step: predictor, right-hand side,
  // S a = g, corrector, and with kinetic / potential the two energies of every level; the body of the three steps calls.
  // CG: S = (1 + gamma dt damp_mass) M + (beta dt^2 + gamma dt damp_stiff) A is built here and every solve synchronises; on
  // a factor (of that S) the whole loop is queued and the stream is waited for once.  D (values NULL: none): the third
  // matrix of the _damped calls; the CG form then adds (gamma dt) D to S in a second combine, in place.  Returns the largest iteration count
  // of a step (0 on a factor) or a negative status.  A record armed on the handle (SlodLodRecord, slod_host.h) is taken
  // first, checked after the call's own checks and queued on st: u and / or v at the receivers after the entry state and
  // every every-th corrector.  A source armed on it (SlodLodSource) is taken with the record, checked after it, and adds
  // one product a step, whose vector the right-hand side reads in place of the load.
  int nm_steps(slod_handle *h, const char *who, SlodLodStepSolve &&solve, const SlodLodOperator &A, const SlodLodOperator &M,
               const SlodLodOperator &D, const uint32_t *d_cols, double dt, double beta, double gamma, double damp_mass, double damp_stiff, int n_steps, int n,
               double *d_u, size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load, size_t ld_load,
               size_t load_step_stride, double *kinetic, double *potential)
  {
    SlodLodRecord rec = slod_lod_record_take(h);
    SlodLodSource src = slod_lod_source_take(h);
    if (const int rc = nm_check(h, who, solve, true, A, M, d_cols && d_u && d_v && d_a, dt, beta, gamma, damp_mass, damp_stiff, n_steps,
                                n, {ld_u, ld_v, ld_a, d_load ? ld_load : ld_u}, (kinetic == nullptr) == (potential == nullptr)))
      return rc;
    if (const int rc = slod_lod_record_check(h, who, &rec, true, n_steps, n, A.per_col))
      return rc;
    if (const int rc = slod_lod_source_check(h, who, src, n_steps + 1, "n_steps + 1", n, A.per_col))
      return rc;
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape w = lod_shape(h, n);
    const bool     energies = kinetic != nullptr;
    const size_t   nmat = solve.cg() ? (size_t)w.NP * w.cap * w.s * w.s : 0, nvec = (size_t)w.nrow * n;
    const size_t   npart = energies ? (size_t)w.ngroup * n : 0, nenergy = energies ? 2 * (size_t)(n_steps + 1) * n : 0;
    // one allocation for the whole loop: S (CG), w = u~ + damp_stiff v~, g, the workspace of the solve, and for the
    // energies two arrays of partials and [level][kinetic, potential][column]; driven by a source, one load
    double    *S, *arg, *g, *part_k, *part_p, *d_energy, *lb;
    hipError_t e = solve.alloc(n, [&](SlodCarver &c) {
      S = c.take(nmat), arg = c.take(nvec), g = c.take(nvec), solve.take(c, h);
      part_k = c.take(npart), part_p = c.take(npart), d_energy = c.take(nenergy), lb = c.take(src.armed ? nvec : 0);
    });
    if (e == hipSuccess)
      {
        const dim3     nblk = lod_flat_grid(nvec);
        const InnerJob jk = inner_job(M, d_v, ld_v, d_v, ld_v, part_k), jp = inner_job(A, d_u, ld_u, d_u, ld_u, part_p);
        const double   gdt = gamma * dt, bdt2 = beta * dt * dt;
        if (solve.cg())
          {
            slod_lod_combine_launch(st, nmat, 1.0 + gdt * damp_mass, M.values, bdt2 + gdt * damp_stiff, A.values, S);
            if (D.values)
              slod_lod_combine_launch(st, nmat, 1.0, S, gdt, D.values, S);
            solve.S = S;
          }
        if (energies)
          launch_inner(w, st, M, d_cols, n, 2, jk, jp, 0.5, d_energy);
        if (rec.armed)
          slod_lod_record_launch(st, rec, 0, n, A.per_col, d_u, ld_u, d_v, ld_v);
        e = hipGetLastError();
        for (int k = 0; k < n_steps && e == hipSuccess; ++k)
          {
            const double *b1 = d_load ? d_load + (size_t)(k + 1) * load_step_stride : nullptr;
            size_t        ld_b = ld_load;
            if (src.armed) // b^(k+1) = the load + O^T g of sample k + 1
              {
                slod_lod_source_launch(st, src, k + 1, 1, n, A.per_col, b1, ld_load, 0, lb, 0);
                b1 = lb, ld_b = (size_t)n;
              }
            hipLaunchKernelGGL(k_nm_predict, nblk, dim3(256), 0, st, w.nrow, n, dt, dt * dt * (0.5 - beta), dt * (1.0 - gamma),
                               damp_stiff, d_u, ld_u, d_v, ld_v, d_a, ld_a, arg);
            launch_rhs(w, st, A, M, D, d_cols, n, damp_mass, b1, ld_b, arg, d_v, ld_v, g);
            e = hipGetLastError();
            if (e == hipSuccess)
              e = solve.solve(h, st, k, n, g, (size_t)n, d_a, ld_a);
            if (e != hipSuccess)
              break;
            hipLaunchKernelGGL(k_nm_correct, nblk, dim3(256), 0, st, w.nrow, n, bdt2, gdt, d_u, ld_u, d_v, ld_v, d_a, ld_a);
            if (energies)
              launch_inner(w, st, M, d_cols, n, 2, jk, jp, 0.5, d_energy + 2 * (size_t)(k + 1) * n);
            if (const int j = rec.slot(k + 1); j >= 0)
              slod_lod_record_launch(st, rec, j, n, A.per_col, d_u, ld_u, d_v, ld_v);
            e = hipGetLastError();
          }
        std::vector<double> host(nenergy);
        if (e == hipSuccess && energies)
          e = hipMemcpyAsync(host.data(), d_energy, nenergy * sizeof(double), hipMemcpyDeviceToHost, st);
        // on every path, a failed one too: the workspace is freed on return and a queued kernel may still touch it
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess)
          e = es;
        if (e == hipSuccess && energies)
          for (size_t k = 0; k <= (size_t)n_steps; ++k)
            for (size_t c = 0; c < (size_t)n; ++c)
              {
                kinetic[k * n + c]   = host[2 * k * n + c];
                potential[k * n + c] = host[(2 * k + 1) * n + c];
              }
      }
    return e == hipSuccess ? solve.work.worst : slod_hip_fail(h, e, who);
  }
} // namespace

// k_lod_inner on the two forms of the energies, then k_lod_inner_sum, for the other time loops of the library
// (slod_lod_irk.hip): the launches and the bits of the energies of nm_steps on one matrix pair, or (per_col) on the
// ensemble matrices with a member per column
void slod_lod_energies_launch(const slod_handle *h, hipStream_t st, const double *d_stiffness, const double *d_mass,
                              const uint32_t *d_cols, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                              double *d_part_k, double *d_part_p, double *d_out, bool per_col, size_t ld_a_m, size_t ld_m_m)
{
  const SlodLodOperator A{d_stiffness, per_col ? ld_a_m : 1, per_col}, M{d_mass, per_col ? ld_m_m : 1, per_col};
  launch_inner(lod_shape(h, n_rhs), st, M, d_cols, n_rhs, 2, inner_job(M, d_v, ld_v, d_v, ld_v, d_part_k),
               inner_job(A, d_u, ld_u, d_u, ld_u, d_part_p), 0.5, d_out);
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_inner_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                         const double *d_y, size_t ld_y, int n_rhs, double *out, void *hip_stream)
{
  return inner(h, "slod_lod_inner_multi", {d_values}, d_cols, d_x, ld_x, d_y, ld_y, n_rhs, out, hip_stream);
}

// slod_lod_inner_multi with a matrix per column: k_lod_inner<true>, then the same ordered sums
int slod_lod_inner_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                            const double *d_y, size_t ld_y, int n_members, double *out, void *hip_stream)
{
  return inner(h, "slod_lod_inner_ensemble", {d_values, ld_m, true}, d_cols, d_x, ld_x, d_y, ld_y, n_members, out, hip_stream);
}

int slod_lod_newmark_accel(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double damp_mass,
                           double damp_stiff, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                           const double *d_load, size_t ld_load, double *d_a, size_t ld_a, double rel_tol, int max_iterations,
                           int *iterations, double *rel_residual)
{
  return nm_accel(h, "slod_lod_newmark_accel", {SLOD_SOLVE_CG, nullptr, d_cols, d_mass, rel_tol, max_iterations}, {d_stiffness}, {d_mass}, {nullptr},
                  d_cols, damp_mass, damp_stiff, n_rhs, d_u, ld_u, d_v, ld_v, d_load, ld_load, d_a, ld_a, iterations, rel_residual);
}

// slod_lod_newmark_accel with the factor of M in place of the CG recurrence
int slod_lod_newmark_accel_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, const double *d_mass,
                                  const uint32_t *d_cols, double damp_mass, double damp_stiff, int n_rhs, const double *d_u, size_t ld_u,
                                  const double *d_v, size_t ld_v, const double *d_load, size_t ld_load, double *d_a, size_t ld_a)
{
  return nm_accel(h, "slod_lod_newmark_accel_direct", {SLOD_SOLVE_FACTOR, f_M}, {d_stiffness}, {d_mass}, {nullptr}, d_cols, damp_mass, damp_stiff,
                  n_rhs, d_u, ld_u, d_v, ld_v, d_load, ld_load, d_a, ld_a);
}

// slod_lod_newmark_accel_direct with a matrix, a factor and a column per member
int slod_lod_newmark_accel_ensemble_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, size_t ld_a_m,
                                           const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, double damp_mass,
                                           double damp_stiff, int n_members, const double *d_u, size_t ld_u, const double *d_v,
                                           size_t ld_v, const double *d_load, size_t ld_load, double *d_a, size_t ld_a)
{
  return nm_accel(h, "slod_lod_newmark_accel_ensemble_direct", {SLOD_SOLVE_FACTOR_PER_COL, f_M}, {d_stiffness, ld_a_m, true},
                  {d_mass, ld_m_m, true}, {nullptr}, d_cols, damp_mass, damp_stiff, n_members, d_u, ld_u, d_v, ld_v, d_load, ld_load, d_a, ld_a);
}

int slod_lod_newmark_steps(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double dt,
                           double beta, double gamma, double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u,
                           size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load, size_t ld_load,
                           size_t load_step_stride, double rel_tol, int max_iterations, int *iterations, double *rel_residual,
                           double *kinetic, double *potential)
{
  return nm_steps(h, "slod_lod_newmark_steps", {SLOD_SOLVE_CG, nullptr, d_cols, nullptr, rel_tol, max_iterations, iterations, rel_residual},
                  {d_stiffness}, {d_mass}, {nullptr}, d_cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_a, ld_a,
                  d_load, ld_load, load_step_stride, kinetic, potential);
}

// slod_lod_newmark_steps with the factor's two sweeps in place of the CG recurrence
int slod_lod_newmark_steps_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const double *d_mass,
                                  const uint32_t *d_cols, double dt, double beta, double gamma, double damp_mass, double damp_stiff,
                                  int n_steps, int n_rhs, double *d_u, size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a,
                                  const double *d_load, size_t ld_load, size_t load_step_stride, double *kinetic, double *potential)
{
  return nm_steps(h, "slod_lod_newmark_steps_direct", {SLOD_SOLVE_FACTOR, f_S}, {d_stiffness}, {d_mass}, {nullptr}, d_cols, dt, beta, gamma,
                  damp_mass, damp_stiff, n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_a, ld_a, d_load, ld_load, load_step_stride, kinetic,
                  potential);
}

// slod_lod_newmark_steps_direct with a matrix, a factor and a column per member
int slod_lod_newmark_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_a_m,
                                           const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, double dt, double beta,
                                           double gamma, double damp_mass, double damp_stiff, int n_steps, int n_members, double *d_u,
                                           size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load,
                                           size_t ld_load, size_t load_step_stride, double *kinetic, double *potential)
{
  return nm_steps(h, "slod_lod_newmark_steps_ensemble_direct", {SLOD_SOLVE_FACTOR_PER_COL, f_S}, {d_stiffness, ld_a_m, true},
                  {d_mass, ld_m_m, true}, {nullptr}, d_cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_members, d_u, ld_u, d_v, ld_v, d_a,
                  ld_a, d_load, ld_load, load_step_stride, kinetic, potential);
}

// The four calls with a third damping matrix, C = damp_mass M + damp_stiff A + D; d_damping NULL: D = 0, the launches and
// the words of the namesake
int slod_lod_newmark_accel_damped(slod_handle *h, const double *d_stiffness, const double *d_mass, const double *d_damping,
                                  const uint32_t *d_cols, double damp_mass, double damp_stiff, int n_rhs, const double *d_u, size_t ld_u,
                                  const double *d_v, size_t ld_v, const double *d_load, size_t ld_load, double *d_a, size_t ld_a,
                                  double rel_tol, int max_iterations, int *iterations, double *rel_residual)
{
  return nm_accel(h, "slod_lod_newmark_accel_damped", {SLOD_SOLVE_CG, nullptr, d_cols, d_mass, rel_tol, max_iterations}, {d_stiffness},
                  {d_mass}, {d_damping}, d_cols, damp_mass, damp_stiff, n_rhs, d_u, ld_u, d_v, ld_v, d_load, ld_load, d_a, ld_a,
                  iterations, rel_residual);
}

int slod_lod_newmark_accel_damped_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, const double *d_mass,
                                         const double *d_damping, const uint32_t *d_cols, double damp_mass, double damp_stiff,
                                         int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                                         const double *d_load, size_t ld_load, double *d_a, size_t ld_a)
{
  return nm_accel(h, "slod_lod_newmark_accel_damped_direct", {SLOD_SOLVE_FACTOR, f_M}, {d_stiffness}, {d_mass}, {d_damping}, d_cols,
                  damp_mass, damp_stiff, n_rhs, d_u, ld_u, d_v, ld_v, d_load, ld_load, d_a, ld_a);
}

int slod_lod_newmark_steps_damped(slod_handle *h, const double *d_stiffness, const double *d_mass, const double *d_damping,
                                  const uint32_t *d_cols, double dt, double beta, double gamma, double damp_mass, double damp_stiff,
                                  int n_steps, int n_rhs, double *d_u, size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a,
                                  const double *d_load, size_t ld_load, size_t load_step_stride, double rel_tol, int max_iterations,
                                  int *iterations, double *rel_residual, double *kinetic, double *potential)
{
  return nm_steps(h, "slod_lod_newmark_steps_damped",
                  {SLOD_SOLVE_CG, nullptr, d_cols, nullptr, rel_tol, max_iterations, iterations, rel_residual}, {d_stiffness}, {d_mass},
                  {d_damping}, d_cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_a, ld_a, d_load,
                  ld_load, load_step_stride, kinetic, potential);
}

int slod_lod_newmark_steps_damped_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const double *d_mass,
                                         const double *d_damping, const uint32_t *d_cols, double dt, double beta, double gamma,
                                         double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                                         double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load, size_t ld_load,
                                         size_t load_step_stride, double *kinetic, double *potential)
{
  return nm_steps(h, "slod_lod_newmark_steps_damped_direct", {SLOD_SOLVE_FACTOR, f_S}, {d_stiffness}, {d_mass}, {d_damping}, d_cols, dt,
                  beta, gamma, damp_mass, damp_stiff, n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_a, ld_a, d_load, ld_load, load_step_stride,
                  kinetic, potential);
}

} // extern "C"
#pragma GCC visibility pop
