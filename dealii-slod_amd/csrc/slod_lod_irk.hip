// Two-stage implicit Runge-Kutta time stepping on the LOD space, one complex solve per step (the reference has no
// counterpart: it solves one stationary problem, LOD.cc:976-1002):
//   slod_lod_irk_coefficients       the pair (alpha, beta) of the step matrix S = alpha A + beta M for
//                                   slod_lod_factor_create_zldl, host only
//   slod_lod_irk_heat_steps_direct  n_steps of  M u' + A u = b(t)
//   slod_lod_irk_wave_steps_direct  n_steps of  M u'' + C u' + A u = b(t),  C = damp_mass M + damp_stiff A
// for the schemes SLOD_IRK_GAUSS2 (order 4, A-stable, conserves the energy of the undamped wave) and SLOD_IRK_RADAU2A
// (order 3, L-stable).  The 2 x 2 Butcher matrix A_rk = T diag(lambda, conj lambda) T^-1 has a complex conjugate pair of
// eigenvalues; for real data the two transformed stage equations are conjugates of each other, so one complex solve with
//   heat  S = M + z A,   wave  S = (1 + z damp_mass) M + (z damp_stiff + z^2) A,   z = dt lambda
// on a member of a complex factor the caller built (slod_lod_factor.hip) carries the step.  With tau the first row of
// T^-1, sigma = tau_1 + tau_2 and mu = b^T T[:,0]:
//   heat  r = tau_1 (b_1 - A u) + tau_2 (b_2 - A u),  S w = r,  u += 2 dt Re(mu w)
//   wave  r = tau_1 b_1 + tau_2 b_2 - sigma [A (u + (z + damp_stiff) v) + damp_mass M v],  S w_v = r,
//         w_u = sigma v + z w_v,  u += 2 dt Re(mu w_u),  v += 2 dt Re(mu w_v)
// b_i the load at t_k + c_i dt.  A step is three launches: the right-hand side (k_irk_heat_rhs, k_irk_wave_rhs: the fma
// chains of slod_lod_apply_multi per row, up to three on one read of the row's column indices, then the complex
// combination), the complex solve of slod_lod_factor_solve_complex out of place into the workspace, and k_irk_advance.
// The energies are k_lod_inner / k_lod_inner_sum of slod_lod_wave.hip (slod_lod_energies_launch).  Both loops are one
// host body (irk_steps), queued whole on the handle's stream and waited for once.  Everything besides the chains is
// elementwise with fp contract off: the bits of a column depend on the factor member, the matrices, the parameters and
// that column alone.
//   slod_lod_irk_damping_coefficient, slod_lod_irk_wave_steps_damped_direct
// add a third matrix to the damping, C = damp_mass M + damp_stiff A + D (a sponge layer): S gains z D (the gamma of
// slod_lod_factor_create_zldl3), the bracket of r gains D v, a fourth chain on the loads of v (DAMP).  Without D the loop
// runs the instantiations and has the words it had before.
//   slod_lod_irk_heat_steps_ensemble_direct, slod_lod_irk_wave_steps_ensemble_direct
// are the same loops with a matrix, a factor member and a column per member of a coefficient ensemble: the right-hand
// side kernels run with PER_COL set (the same chains on member m's words of the member-minor ensemble matrices, their
// loads issued LOD_SLOTS slots ahead), the solve launches member first_member + m on column m, k_irk_advance serves as
// it is, and the energies are k_lod_inner<true>.  Column m keeps the words of the single call on member m.
#include "slod_lod_tile.hip.h"

#include <cmath>
#include <complex>
#include <vector>

namespace
{
  // The constants of a scheme on a step, as the kernels take them: every complex number as (re, im).
  struct IrkStep
  {
    double t1r, t1i, t2r, t2i; // tau
    double sr, si;             // sigma
    double zr, zi;             // z = dt lambda
    double zdr;                // Re z + damp_stiff: the factor of A v in the wave's right-hand side
    double cr, ci;             // 2 dt mu
    double damp_mass;
  };

  // The row's chains in one walk over its slots: acc[0] = (A x0)_i and, as far as asked for, acc[1] = (A x1)_i and
  // acc[2] = (M x1)_i, every one the fma chain of slod_lod_row_product on its own operands.  DAMP (NCHAIN >= 2): the
  // fourth chain acc[3] = (D x1)_i of the third matrix dm, on the same loads of x1.
  template <int NCHAIN, bool DAMP>
  __device__ __forceinline__ void irk_row_products(int i, int s, int cap, int NP, const double *__restrict__ a,
                                                   const double *__restrict__ m, const double *__restrict__ dm,
                                                   const uint32_t *__restrict__ cols, const double *__restrict__ x0, size_t ld0,
                                                   const double *__restrict__ x1, size_t ld1, int col, double (&acc)[4])
  {
    const int    p = i / s, d = i - p * s;
    const size_t slot0 = (size_t)p * cap;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    for (int j = 0; j < cap; ++j)
      {
        const uint32_t q = cols[slot0 + j];
        const bool     used = q < (uint32_t)NP;
        const size_t   qs = (size_t)(used ? q : (uint32_t)p) * s, at = (slot0 + j) * s * s + d * s;
        for (int e = 0; e < s; ++e)
          {
            const double t0 = fma(a[at + e], x0[(qs + e) * ld0 + col], acc[0]);
            acc[0]          = used ? t0 : acc[0];
            if constexpr (NCHAIN >= 2)
              {
                const double xv = x1[(qs + e) * ld1 + col];
                const double t1 = fma(a[at + e], xv, acc[1]);
                acc[1]          = used ? t1 : acc[1];
                if constexpr (NCHAIN >= 3)
                  {
                    const double t2 = fma(m[at + e], xv, acc[2]);
                    acc[2]          = used ? t2 : acc[2];
                  }
                if constexpr (DAMP)
                  {
                    const double t3 = fma(dm[at + e], xv, acc[3]);
                    acc[3]          = used ? t3 : acc[3];
                  }
              }
          }
      }
  }

  // The same chains with a matrix per column on the one pattern (the ensemble layout of include/slod.h): entry e of
  // column col's matrices at a[e ld_a + col] and m[e ld_m + col].  Every (row, column) streams its own matrix words, so,
  // as in slod_lod_row_product_per_col, the loads of SLOTS slots are issued before the first fma needs one: every word of
  // A once for the chains on x0 and x1, the words of M in the same batch when the mass chain runs.  A slot past the end
  // of the row reads the last one and adds nothing, like an unused slot.  DAMP: the words of the third matrix dm (ld_d) in
  // the same batch, for the chain acc[3].
  template <int NCHAIN, bool DAMP, int S, int SLOTS> // S = s, a constant here so that nothing stands between the loads
  __device__ __forceinline__ void irk_row_products_per_col(int p, int d, int cap, int NP, const double *__restrict__ a, size_t ld_a,
                                                           const double *__restrict__ m, size_t ld_m, const double *__restrict__ dm,
                                                           size_t ld_d, const uint32_t *__restrict__ cols,
                                                           const double *__restrict__ x0, size_t ld0, const double *__restrict__ x1,
                                                           size_t ld1, int col, double (&acc)[4])
  {
    const size_t slot0 = (size_t)p * cap;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    for (int j0 = 0; j0 < cap; j0 += SLOTS)
      {
        bool   used[SLOTS];
        double aw[SLOTS][S], mw[NCHAIN >= 3 ? SLOTS : 1][S], xu[SLOTS][S], xv[NCHAIN >= 2 ? SLOTS : 1][S];
        double dw[DAMP ? SLOTS : 1][S];
#pragma unroll
        for (int u = 0; u < SLOTS; ++u)
          {
            const int      j = min(j0 + u, cap - 1);
            const uint32_t q = cols[slot0 + j];
            used[u]          = q < (uint32_t)NP && j0 + u < cap;
            const size_t qs = (size_t)(used[u] ? q : (uint32_t)p) * S, at = (slot0 + j) * S * S + d * S;
#pragma unroll
            for (int e = 0; e < S; ++e)
              {
                aw[u][e] = a[(at + e) * ld_a + col];
                xu[u][e] = x0[(qs + e) * ld0 + col];
                if constexpr (NCHAIN >= 2)
                  xv[u][e] = x1[(qs + e) * ld1 + col];
                if constexpr (NCHAIN >= 3)
                  mw[u][e] = m[(at + e) * ld_m + col];
                if constexpr (DAMP)
                  dw[u][e] = dm[(at + e) * ld_d + col];
              }
          }
#pragma unroll
        for (int u = 0; u < SLOTS; ++u)
#pragma unroll
          for (int e = 0; e < S; ++e)
            {
              const double t0 = fma(aw[u][e], xu[u][e], acc[0]);
              acc[0]          = used[u] ? t0 : acc[0];
              if constexpr (NCHAIN >= 2)
                {
                  const double t1 = fma(aw[u][e], xv[u][e], acc[1]);
                  acc[1]          = used[u] ? t1 : acc[1];
                  if constexpr (NCHAIN >= 3)
                    {
                      const double t2 = fma(mw[u][e], xv[u][e], acc[2]);
                      acc[2]          = used[u] ? t2 : acc[2];
                    }
                  if constexpr (DAMP)
                    {
                      const double t3 = fma(dw[u][e], xv[u][e], acc[3]);
                      acc[3]          = used[u] ? t3 : acc[3];
                    }
                }
            }
      }
  }

  // The chains of row i for column col: on the one matrix pair, or (PER_COL) on member col of the ensemble matrices
  template <int NCHAIN, bool PER_COL, bool DAMP = false>
  __device__ __forceinline__ void irk_products(int i, int s, int cap, int NP, const double *__restrict__ a, size_t ld_a,
                                               const double *__restrict__ m, size_t ld_m, const double *__restrict__ dm, size_t ld_d,
                                               const uint32_t *__restrict__ cols, const double *__restrict__ x0, size_t ld0,
                                               const double *__restrict__ x1, size_t ld1, int col, double (&acc)[4])
  {
    static_assert(!DAMP || NCHAIN >= 2, "the damping chain runs on the loads of x1");
    if constexpr (PER_COL)
      {
        const int p = i / s, d = i - p * s;
        if (s == 1)
          irk_row_products_per_col<NCHAIN, DAMP, 1, LOD_SLOTS>(p, d, cap, NP, a, ld_a, m, ld_m, dm, ld_d, cols, x0, ld0, x1, ld1, col,
                                                               acc);
        else
          irk_row_products_per_col<NCHAIN, DAMP, 2, LOD_SLOTS>(p, d, cap, NP, a, ld_a, m, ld_m, dm, ld_d, cols, x0, ld0, x1, ld1, col,
                                                               acc);
      }
    else
      irk_row_products<NCHAIN, DAMP>(i, s, cap, NP, a, m, dm, cols, x0, ld0, x1, ld1, col, acc);
  }

  // r = tau_1 (b_1 - A u) + tau_2 (b_2 - A u) per (row, column), both planes; b1 NULL: zero load.  PER_COL: column c
  // reads member c of the ensemble matrix stiffness (ld_a_m).
  template <bool PER_COL>
  __global__ __launch_bounds__(256) void k_irk_heat_rhs(int nrow, int s, int cap, int NP, int n_rhs, IrkStep k,
                                                       const double *__restrict__ stiffness, size_t ld_a_m,
                                                       const uint32_t *__restrict__ cols, const double *b1, const double *b2,
                                                       size_t ld_b, const double *u, size_t ld_u, double *r_re, double *r_im)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const int i = (int)(t / n_rhs), c = (int)(t - (size_t)i * n_rhs);
    double    acc[4];
    irk_products<1, PER_COL>(i, s, cap, NP, stiffness, ld_a_m, nullptr, 0, nullptr, 0, cols, u, ld_u, nullptr, 0, c, acc);
    const double d1 = (b1 ? b1[(size_t)i * ld_b + c] : 0.0) - acc[0], d2 = (b1 ? b2[(size_t)i * ld_b + c] : 0.0) - acc[0];
    const double p1r = k.t1r * d1, p2r = k.t2r * d2, p1i = k.t1i * d1, p2i = k.t2i * d2;
    r_re[t] = p1r + p2r;
    r_im[t] = p1i + p2i;
  }

  // r = tau_1 b_1 + tau_2 b_2 - sigma [A u + (z + damp_stiff) A v + damp_mass M v] per (row, column), both planes;
  // b1 NULL: zero load.  HAS_MASS_DAMPING unset: no mass chain (damp_mass = 0).  PER_COL: column c reads member c of the
  // ensemble matrices stiffness (ld_a_m) and mass (ld_m_m).  HAS_DAMPING: the bracket gains D v of the third matrix
  // damping (ld_d_m), added after the mass term.
  template <bool HAS_MASS_DAMPING, bool PER_COL, bool HAS_DAMPING = false>
  __global__ __launch_bounds__(256) void k_irk_wave_rhs(int nrow, int s, int cap, int NP, int n_rhs, IrkStep k,
                                                       const double *__restrict__ stiffness, size_t ld_a_m,
                                                       const double *__restrict__ mass, size_t ld_m_m,
                                                       const double *__restrict__ damping, size_t ld_d_m,
                                                       const uint32_t *__restrict__ cols, const double *b1, const double *b2,
                                                       size_t ld_b, const double *u, size_t ld_u, const double *v, size_t ld_v,
                                                       double *r_re, double *r_im)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const int i = (int)(t / n_rhs), c = (int)(t - (size_t)i * n_rhs);
    double    acc[4];
    irk_products<HAS_MASS_DAMPING ? 3 : 2, PER_COL, HAS_DAMPING>(i, s, cap, NP, stiffness, ld_a_m, mass, ld_m_m, damping, ld_d_m, cols,
                                                                 u, ld_u, v, ld_v, c, acc);
    // p = A u + (z + damp_stiff) A v + damp_mass M v [+ D v]
    const double av_r = k.zdr * acc[1];
    double       pr = acc[0] + av_r;
    const double pi = k.zi * acc[1];
    if constexpr (HAS_MASS_DAMPING)
      {
        const double dm = k.damp_mass * acc[2];
        pr              = pr + dm;
      }
    if constexpr (HAS_DAMPING)
      pr = pr + acc[3];
    // sigma p, complex product written out
    const double a = k.sr * pr, b = k.si * pi, e = k.sr * pi, f = k.si * pr;
    const double qr = a - b, qi = e + f;
    double       lr = 0.0, li = 0.0;
    if (b1)
      {
        const double x1 = b1[(size_t)i * ld_b + c], x2 = b2[(size_t)i * ld_b + c];
        const double p1r = k.t1r * x1, p2r = k.t2r * x2, p1i = k.t1i * x1, p2i = k.t2i * x2;
        lr = p1r + p2r, li = p1i + p2i;
      }
    r_re[t] = lr - qr;
    r_im[t] = li - qi;
  }

  // The damping chain with a matrix per column has no entry point yet; instantiated here so that it keeps compiling and an
  // ensemble form of the damped call is a launch.
  template __global__ void k_irk_wave_rhs<true, true, true>(int, int, int, int, int, IrkStep, const double *, size_t, const double *,
                                                            size_t, const double *, size_t, const uint32_t *, const double *,
                                                            const double *, size_t, const double *, size_t, const double *, size_t,
                                                            double *, double *);
  template __global__ void k_irk_wave_rhs<false, true, true>(int, int, int, int, int, IrkStep, const double *, size_t, const double *,
                                                             size_t, const double *, size_t, const uint32_t *, const double *,
                                                             const double *, size_t, const double *, size_t, const double *, size_t,
                                                             double *, double *);

  // ORDER 1:  u += 2 dt Re(mu w).  ORDER 2:  w_u = sigma v + z w,  u += 2 dt Re(mu w_u),  v += 2 dt Re(mu w).
  template <int ORDER>
  __global__ __launch_bounds__(256) void k_irk_advance(int nrow, int n_rhs, IrkStep k, const double *w_re, const double *w_im,
                                                      double *u, size_t ld_u, double *v, size_t ld_v)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n_rhs)
      return;
    const size_t i = t / n_rhs, c = t - i * n_rhs;
    const double wr = w_re[t], wi = w_im[t];
    const double a = k.cr * wr, b = k.ci * wi;
    const double dw = a - b; // 2 dt Re(mu w)
    if constexpr (ORDER == 1)
      u[i * ld_u + c] = u[i * ld_u + c] + dw;
    else
      {
        const double vi = v[i * ld_v + c];
        const double zr1 = k.zr * wr, zr2 = k.zi * wi, zi1 = k.zr * wi, zi2 = k.zi * wr;
        const double sv_r = k.sr * vi, sv_i = k.si * vi;
        const double ur = sv_r + (zr1 - zr2), ui = sv_i + (zi1 + zi2);
        const double e = k.cr * ur, f = k.ci * ui;
        const double du = e - f;
        u[i * ld_u + c] = u[i * ld_u + c] + du;
        v[i * ld_v + c] = vi + dw;
      }
  }

  using cld = std::complex<long double>;

  // lambda (positive imaginary part), tau, sigma and mu of a scheme, in long double: the eigenvector of lambda is
  // t = (a_12, lambda - a_11), T = [t, conj t], and the first row of T^-1 is (conj t_2, -conj t_1) / det T.
  struct IrkScheme
  {
    cld lambda, tau1, tau2, sigma, mu;
  };
  bool irk_scheme(int scheme, IrkScheme *out)
  {
    const long double r3 = std::sqrt(3.0L), r2 = std::sqrt(2.0L);
    long double       a11, a12, b1, b2;
    if (scheme == SLOD_IRK_GAUSS2)
      a11 = 0.25L, a12 = 0.25L - r3 / 6.0L, b1 = 0.5L, b2 = 0.5L, out->lambda = cld(0.25L, r3 / 12.0L);
    else if (scheme == SLOD_IRK_RADAU2A)
      a11 = 5.0L / 12.0L, a12 = -1.0L / 12.0L, b1 = 0.75L, b2 = 0.25L, out->lambda = cld(1.0L / 3.0L, r2 / 6.0L);
    else
      return false;
    const cld t1(a12, 0.0L), t2 = out->lambda - a11;
    const cld det = t1 * std::conj(t2) - std::conj(t1) * t2;
    out->tau1     = std::conj(t2) / det;
    out->tau2     = -std::conj(t1) / det;
    out->sigma    = out->tau1 + out->tau2;
    out->mu       = b1 * t1 + b2 * t2;
    return true;
  }

  IrkStep irk_step(const IrkScheme &s, double dt, double damp_mass, double damp_stiff)
  {
    const cld z = (long double)dt * s.lambda, c = 2.0L * (long double)dt * s.mu;
    IrkStep   k;
    k.t1r = (double)s.tau1.real(), k.t1i = (double)s.tau1.imag(), k.t2r = (double)s.tau2.real(), k.t2i = (double)s.tau2.imag();
    k.sr = (double)s.sigma.real(), k.si = (double)s.sigma.imag();
    k.zr = (double)z.real(), k.zi = (double)z.imag();
    k.zdr = (double)(z.real() + (long double)damp_stiff);
    k.cr = (double)c.real(), k.ci = (double)c.imag();
    k.damp_mass = damp_mass;
    return k;
  }

  // n_steps of a two-stage scheme on n columns, heat (order 1: d_v, d_mass, the dampings and the energies are not used)
  // or wave (order 2); the body of the four calls.  Single: the n = n_rhs columns on the one matrix pair and on factor
  // member first_member.  per_col: column m on member m of the ensemble matrices (ld_a_m, ld_m_m) and on factor member
  // first_member + m, which reads column m of the right-hand side whatever first_member.  The whole loop is queued and
  // the stream is waited for once: three launches a step, five with the energies, for any n.  A record armed on the
  // handle (SlodLodRecord, slod_host.h) is taken first, checked after the call's own checks and adds one launch after the
  // entry state and every every-th advance.  A source armed on it (SlodLodSource) is taken with the record, checked after
  // it, and adds one launch a step, whose two vectors the right-hand side reads in place of the stage loads.
  // d_damping (wave; NULL: none): the third matrix D of the _damped call, on a factor of S + z D.
  int irk_steps(slod_handle *h, const std::string &who, int order, slod_lod_factor *f, int first_member, int scheme,
                const double *d_stiffness, size_t ld_a_m, const double *d_mass, size_t ld_m_m, const double *d_damping, size_t ld_d_m,
                bool per_col, const uint32_t *d_cols,
                double dt, double damp_mass, double damp_stiff, int n_steps, int n, double *d_u, size_t ld_u, double *d_v, size_t ld_v,
                const double *d_load, size_t ld_load, size_t load_stage_stride, double *kinetic, double *potential)
  {
    const bool    wave = order == 2;
    SlodLodRecord rec = slod_lod_record_take(h);
    SlodLodSource src = slod_lod_source_take(h);
    if (!h)
      return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL handle");
    if (!d_stiffness || !d_cols || !d_u || (wave && (!d_mass || !d_v)))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL matrix, d_cols or state");
    IrkScheme sch;
    if (!irk_scheme(scheme, &sch))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": unknown scheme");
    if (!(dt > 0.0) || std::isinf(dt))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": dt <= 0, NaN or infinite");
    if (!(damp_mass >= 0.0) || !(damp_stiff >= 0.0) || std::isinf(damp_mass) || std::isinf(damp_stiff))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": negative, NaN or infinite damping coefficient");
    if (n_steps < 1 || n < 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (per_col ? ": n_steps < 1 or n_members < 1" : ": n_steps < 1 or n_rhs < 1"));
    if (const int rc = slod_check_ld_of(h, who.c_str(), per_col, {ld_a_m, wave ? ld_m_m : ld_a_m}, n,
                                        {ld_u, wave ? ld_v : ld_u, d_load ? ld_load : ld_u}))
      return rc;
    if ((kinetic == nullptr) != (potential == nullptr))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": kinetic and potential come together or not at all");
    if (!f)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL factor");
    if (f->h != h || f->n != h->NP * h->cfg.spacedim)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": factor of another handle / row count");
    if (f->kind != SLOD_FACTOR_ZLDL)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": takes a complex factor (slod_lod_factor_create_zldl)");
    const int n_fm = per_col ? n : 1; // factor members of the call
    if (first_member < 0 || first_member > f->n_members - n_fm)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (per_col ? ": members outside the factor" : ": member outside the factor"));
    if (const int rc = slod_lod_record_check(h, who, &rec, wave, n_steps, n, per_col))
      return rc;
    if (const int rc = slod_lod_source_check(h, who, src, 2 * n_steps, "2 n_steps", n, per_col))
      return rc;
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape w = lod_shape(h, n);
    const IrkStep  k = irk_step(sch, dt, damp_mass, damp_stiff);
    const bool     energies = wave && kinetic != nullptr;
    const size_t   nvec = (size_t)w.nrow * n, npart = energies ? (size_t)w.ngroup * n : 0;
    const size_t   nenergy = energies ? 2 * (size_t)(n_steps + 1) * n : 0;
    // one allocation for the whole loop: the two planes of r and of w, and for the energies two arrays of partials and
    // [level][kinetic, potential][column]; driven by a source, the two stage loads
    SlodDevBuf<double> work;
    hipError_t         e = work.alloc(4 * nvec + 2 * npart + nenergy + (src.armed ? 2 * nvec : 0));
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who.c_str());
    double *r_re = work.get(), *r_im = r_re + nvec, *w_re = r_im + nvec, *w_im = w_re + nvec;
    double *part_k = w_im + nvec, *part_p = part_k + npart, *d_energy = part_p + npart, *lb = d_energy + nenergy;
    const dim3     nblk = lod_flat_grid(nvec);
    const auto     heat_rhs = per_col ? k_irk_heat_rhs<true> : k_irk_heat_rhs<false>;
    const auto     wave_rhs = d_damping && !per_col ? (damp_mass != 0.0 ? k_irk_wave_rhs<true, false, true> : k_irk_wave_rhs<false, false, true>)
                              : damp_mass != 0.0    ? (per_col ? k_irk_wave_rhs<true, true> : k_irk_wave_rhs<true, false>)
                                                    : (per_col ? k_irk_wave_rhs<false, true> : k_irk_wave_rhs<false, false>);
    auto launch_energies = [&](int level) {
      slod_lod_energies_launch(h, st, d_stiffness, d_mass, d_cols, n, d_u, ld_u, d_v, ld_v, part_k, part_p,
                               d_energy + 2 * (size_t)level * n, per_col, ld_a_m, ld_m_m);
    };
    if (energies)
      launch_energies(0);
    if (rec.armed)
      slod_lod_record_launch(st, rec, 0, n, per_col, d_u, ld_u, d_v, ld_v);
    e = hipGetLastError();
    for (int step = 0; step < n_steps && e == hipSuccess; ++step)
      {
        const double *b1 = d_load ? d_load + (size_t)(2 * step) * load_stage_stride : nullptr;
        const double *b2 = d_load ? d_load + ((size_t)(2 * step) + 1) * load_stage_stride : nullptr;
        size_t        ld_b = ld_load;
        if (src.armed) // the two stage loads + O^T g of the samples 2 step and 2 step + 1, in one launch
          {
            slod_lod_source_launch(st, src, 2 * step, 2, n, per_col, b1, ld_load, load_stage_stride, lb, nvec);
            b1 = lb, b2 = lb + nvec, ld_b = (size_t)n;
          }
        if (!wave)
          hipLaunchKernelGGL(heat_rhs, nblk, dim3(256), 0, st, w.nrow, w.s, w.cap, w.NP, n, k, d_stiffness, ld_a_m, d_cols, b1, b2,
                             ld_b, d_u, ld_u, r_re, r_im);
        else
          hipLaunchKernelGGL(wave_rhs, nblk, dim3(256), 0, st, w.nrow, w.s, w.cap, w.NP, n, k, d_stiffness, ld_a_m, d_mass, ld_m_m,
                             d_damping, ld_d_m, d_cols, b1, b2, ld_b, d_u, ld_u, d_v, ld_v, r_re, r_im);
        // single: the n columns on the one member; per_col: member first_member + m on column m of r, one column each
        if (per_col)
          slod_lod_zfactor_solve_launch(f, st, first_member, n, r_re, r_im, (size_t)n, 1, 0, n, w_re, w_im, (size_t)n);
        else
          slod_lod_zfactor_solve_launch(f, st, first_member, 1, r_re, r_im, (size_t)n, n, 0, 1, w_re, w_im, (size_t)n);
        if (!wave)
          hipLaunchKernelGGL(k_irk_advance<1>, nblk, dim3(256), 0, st, w.nrow, n, k, w_re, w_im, d_u, ld_u, nullptr, 0);
        else
          hipLaunchKernelGGL(k_irk_advance<2>, nblk, dim3(256), 0, st, w.nrow, n, k, w_re, w_im, d_u, ld_u, d_v, ld_v);
        if (energies)
          launch_energies(step + 1);
        if (const int j = rec.slot(step + 1); j >= 0)
          slod_lod_record_launch(st, rec, j, n, per_col, d_u, ld_u, d_v, ld_v);
        e = hipGetLastError();
      }
    std::vector<double> host(nenergy);
    if (e == hipSuccess && energies)
      e = hipMemcpyAsync(host.data(), d_energy, nenergy * sizeof(double), hipMemcpyDeviceToHost, st);
    // on every path, a failed one too: the workspace is freed on return and a queued kernel may still touch it
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess)
      e = es;
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who.c_str());
    if (energies)
      for (size_t l = 0; l <= (size_t)n_steps; ++l)
        for (size_t c = 0; c < (size_t)n; ++c)
          {
            kinetic[l * n + c]   = host[2 * l * n + c];
            potential[l * n + c] = host[(2 * l + 1) * n + c];
          }
    return SLOD_OK;
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_irk_coefficients(int scheme, int order, double dt, double damp_mass, double damp_stiff, double alpha[2], double beta[2])
{
  const std::string who = "slod_lod_irk_coefficients";
  IrkScheme         s;
  if (!alpha || !beta)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL alpha or beta");
  if (!irk_scheme(scheme, &s))
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": unknown scheme");
  if (order != 1 && order != 2)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": order is 1 (heat) or 2 (wave)");
  if (!(dt > 0.0) || std::isinf(dt))
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": dt <= 0, NaN or infinite");
  if (!(damp_mass >= 0.0) || !(damp_stiff >= 0.0) || std::isinf(damp_mass) || std::isinf(damp_stiff))
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": negative, NaN or infinite damping coefficient");
  if (order == 1 && (damp_mass != 0.0 || damp_stiff != 0.0))
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": a damping coefficient with order 1 (heat)");
  const cld z = (long double)dt * s.lambda;
  const cld a = order == 1 ? z : z * (long double)damp_stiff + z * z, b = order == 1 ? cld(1.0L) : 1.0L + z * (long double)damp_mass;
  alpha[0] = (double)a.real(), alpha[1] = (double)a.imag();
  beta[0] = (double)b.real(), beta[1] = (double)b.imag();
  for (const double x : {alpha[0], alpha[1], beta[0], beta[1]})
    if (!std::isfinite(x))
      return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": dt^2 or dt times a damping coefficient overflows");
  return SLOD_OK;
}

int slod_lod_irk_heat_steps_direct(slod_handle *h, slod_lod_factor *f_S, int member, int scheme, const double *d_stiffness,
                                   const uint32_t *d_cols, double dt, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                                   const double *d_load, size_t ld_load, size_t load_stage_stride)
{
  return irk_steps(h, "slod_lod_irk_heat_steps_direct", 1, f_S, member, scheme, d_stiffness, 1, nullptr, 1, nullptr, 1, false, d_cols, dt, 0.0, 0.0,
                   n_steps, n_rhs, d_u, ld_u, nullptr, 0, d_load, ld_load, load_stage_stride, nullptr, nullptr);
}

int slod_lod_irk_wave_steps_direct(slod_handle *h, slod_lod_factor *f_S, int member, int scheme, const double *d_stiffness,
                                   const double *d_mass, const uint32_t *d_cols, double dt, double damp_mass, double damp_stiff,
                                   int n_steps, int n_rhs, double *d_u, size_t ld_u, double *d_v, size_t ld_v, const double *d_load,
                                   size_t ld_load, size_t load_stage_stride, double *kinetic, double *potential)
{
  return irk_steps(h, "slod_lod_irk_wave_steps_direct", 2, f_S, member, scheme, d_stiffness, 1, d_mass, 1, nullptr, 1, false, d_cols, dt, damp_mass,
                   damp_stiff, n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_load, ld_load, load_stage_stride, kinetic, potential);
}

// gamma = z = dt lambda of the scheme, the coefficient of D in the step matrix of the damped wave
int slod_lod_irk_damping_coefficient(int scheme, double dt, double gamma[2])
{
  const std::string who = "slod_lod_irk_damping_coefficient";
  IrkScheme         s;
  if (!gamma)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL gamma");
  if (!irk_scheme(scheme, &s))
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": unknown scheme");
  if (!(dt > 0.0) || std::isinf(dt))
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": dt <= 0, NaN or infinite");
  const cld z = (long double)dt * s.lambda;
  gamma[0] = (double)z.real(), gamma[1] = (double)z.imag();
  return SLOD_OK;
}

// slod_lod_irk_wave_steps_direct with the third damping matrix D, on a member of the factor of S + z D
// (slod_lod_factor_create_zldl3); d_damping NULL: D = 0, the launches and the words of slod_lod_irk_wave_steps_direct
int slod_lod_irk_wave_steps_damped_direct(slod_handle *h, slod_lod_factor *f_S, int member, int scheme, const double *d_stiffness,
                                          const double *d_mass, const double *d_damping, const uint32_t *d_cols, double dt,
                                          double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                                          double *d_v, size_t ld_v, const double *d_load, size_t ld_load, size_t load_stage_stride,
                                          double *kinetic, double *potential)
{
  return irk_steps(h, "slod_lod_irk_wave_steps_damped_direct", 2, f_S, member, scheme, d_stiffness, 1, d_mass, 1, d_damping, 1, false,
                   d_cols, dt, damp_mass, damp_stiff, n_steps, n_rhs, d_u, ld_u, d_v, ld_v, d_load, ld_load, load_stage_stride, kinetic,
                   potential);
}

// slod_lod_irk_heat_steps_direct with a matrix, a factor member and a column per ensemble member
int slod_lod_irk_heat_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, int first_member, int scheme,
                                            const double *d_stiffness, size_t ld_a_m, const uint32_t *d_cols, double dt, int n_steps,
                                            int n_members, double *d_u, size_t ld_u, const double *d_load, size_t ld_load,
                                            size_t load_stage_stride)
{
  return irk_steps(h, "slod_lod_irk_heat_steps_ensemble_direct", 1, f_S, first_member, scheme, d_stiffness, ld_a_m, nullptr, ld_a_m, nullptr, 1, true,
                   d_cols, dt, 0.0, 0.0, n_steps, n_members, d_u, ld_u, nullptr, 0, d_load, ld_load, load_stage_stride, nullptr, nullptr);
}

// slod_lod_irk_wave_steps_direct with a matrix pair, a factor member and a column per ensemble member
int slod_lod_irk_wave_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, int first_member, int scheme,
                                            const double *d_stiffness, size_t ld_a_m, const double *d_mass, size_t ld_m_m,
                                            const uint32_t *d_cols, double dt, double damp_mass, double damp_stiff, int n_steps,
                                            int n_members, double *d_u, size_t ld_u, double *d_v, size_t ld_v, const double *d_load,
                                            size_t ld_load, size_t load_stage_stride, double *kinetic, double *potential)
{
  return irk_steps(h, "slod_lod_irk_wave_steps_ensemble_direct", 2, f_S, first_member, scheme, d_stiffness, ld_a_m, d_mass, ld_m_m, nullptr, 1, true,
                   d_cols, dt, damp_mass, damp_stiff, n_steps, n_members, d_u, ld_u, d_v, ld_v, d_load, ld_load, load_stage_stride,
                   kinetic, potential);
}

} // extern "C"
#pragma GCC visibility pop
