// The frequency response on the LOD space: for  M u'' + C u' + A u = Re(b e^{i omega t}),  C = damp_mass M + damp_stiff A
// (the Rayleigh damping of the Newmark calls), the amplitude solves the complex symmetric system
//   S(omega) u = b,   S(omega) = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M.
//   slod_lod_harmonic_response   a sweep of frequencies in one call: frequency k is member k of a complex banded LDL^T
//                                (slod_lod_factor_create_zldl, slod_lod_factor.hip) with alpha_k = (1, omega_k damp_stiff),
//                                beta_k = (-(omega_k omega_k), omega_k damp_mass), solved on the shared load; then the true
//                                residual from the matrices themselves and the growth of every factor
// The sweep runs in chunks of at most HARMONIC_CHUNK frequencies (one factor allocation each), every chunk queued whole on
// the handle's stream and waited for once.  A member's bits do not depend on the members beside it, so the result does
// not depend on the chunking.
// Residual: the four products A u_re, A u_im, M u_re, M u_im by the fma chain of slod_lod_apply_multi, combined per entry
// with the complex coefficients (k_harmonic_residual: every product and sum rounded on its own, in one order), squared and
// summed over the rows of a group, then over the groups, both ascending (slod_lod_tile.hip.h): no atomics.
#include "slod_lod_tile.hip.h"

#include <cmath>
#include <vector>

namespace
{
  constexpr int HARMONIC_CHUNK = 64; // frequencies per factor allocation

  // partial[g][col] = sum over the rows of group g of |r|^2, r = b - ((alpha A + beta M) u) of column col = k n_rhs + c
  // (frequency k of the chunk, load column c);  partial_b[g][col] the same of |b|^2.  coef: [members][4] of the factor.
  __global__ __launch_bounds__(LOD_BLOCK) void k_harmonic_residual(int nrow, int n_rhs, int ncol, int ngroup, const double *__restrict__ coef,
                                                                 const double *__restrict__ au_re, const double *__restrict__ au_im,
                                                                 const double *__restrict__ mu_re, const double *__restrict__ mu_im,
                                                                 const double *__restrict__ b_re, const double *__restrict__ b_im,
                                                                 size_t ld_b, double *__restrict__ partial, double *__restrict__ partial_b)
  {
#pragma clang fp contract(off)
    __shared__ double sR[LOD_ROWS][LOD_COLS], sB[LOD_ROWS][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, ncol - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    rr = 0.0, bb = 0.0;
            if (i < nrow)
              {
                const int     k = col / n_rhs, lc = col - k * n_rhs;
                const double *ck = coef + 4 * k;
                const size_t  at = (size_t)i * ncol + col;
                const double  ar = au_re[at], ai = au_im[at], mr = mu_re[at], mi = mu_im[at];
                const double  br = b_re[(size_t)i * ld_b + lc], bi = b_im ? b_im[(size_t)i * ld_b + lc] : 0.0;
                // S u = alpha (A u) + beta (M u), complex products written out
                const double sr = ((ck[0] * ar - ck[1] * ai) + (ck[2] * mr - ck[3] * mi));
                const double si = ((ck[0] * ai + ck[1] * ar) + (ck[2] * mi + ck[3] * mr));
                const double er = br - sr, ei = bi - si;
                rr = er * er + ei * ei;
                bb = br * br + bi * bi;
              }
            sR[lr][c] = rr, sB[lr][c] = bb;
          }
        __syncthreads();
        if ((int)threadIdx.x < nb)
          {
            partial[(size_t)g * ncol + c0 + threadIdx.x]   = slod_lod_group_sum(sR, threadIdx.x);
            partial_b[(size_t)g * ncol + c0 + threadIdx.x] = slod_lod_group_sum(sB, threadIdx.x);
          }
        __syncthreads();
      }
  }

  // out[col] = ||r||_2 / ||b||_2, the groups summed in ascending order; a zero load column gives 0
  __global__ __launch_bounds__(LOD_BLOCK) void k_harmonic_norms(int ncol, int ngroup, const double *__restrict__ partial,
                                                              const double *__restrict__ partial_b, double *__restrict__ out)
  {
    const int col = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (col >= ncol)
      return;
    const double rr = slod_lod_ordered_sum(partial, ngroup, ncol, col), bb = slod_lod_ordered_sum(partial_b, ngroup, ncol, col);
    out[col] = bb > 0.0 ? sqrt(rr) / sqrt(bb) : (rr > 0.0 ? HUGE_VAL : 0.0);
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" int slod_lod_harmonic_response(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                                          double damp_mass, double damp_stiff, const double *omega, int n_freq, const double *d_load_re,
                                          const double *d_load_im, size_t ld_load, int n_rhs, double *d_u_re, double *d_u_im,
                                          size_t ld_u, double *rel_residual, double *growth)
{
  const std::string who = "slod_lod_harmonic_response";
  if (!h || !d_stiffness || !d_mass || !d_cols || !omega || !d_load_re || !d_u_re || !d_u_im)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL handle, matrix, d_cols, omega, load or u");
  if (!(damp_mass >= 0.0) || !(damp_stiff >= 0.0) || std::isinf(damp_mass) || std::isinf(damp_stiff))
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": negative, NaN or infinite damping coefficient");
  if (n_freq < 1 || n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_freq < 1 or n_rhs < 1");
  for (int k = 0; k < n_freq; ++k)
    if (!(omega[k] >= 0.0) || std::isinf(omega[k]))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": a frequency is negative, NaN or infinite");
  if (ld_load < (size_t)n_rhs)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of the load below n_rhs");
  if (ld_u / (size_t)n_rhs < (size_t)n_freq)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of u below n_freq * n_rhs");
  // (-(omega omega), omega damp) must be finite for the factor
  std::vector<double> alpha(2 * (size_t)n_freq), beta(2 * (size_t)n_freq);
  for (int k = 0; k < n_freq; ++k)
    {
      const double w = omega[k];
      alpha[2 * k] = 1.0, alpha[2 * k + 1] = w * damp_stiff;
      beta[2 * k] = -(w * w), beta[2 * k + 1] = w * damp_mass;
      if (!std::isfinite(alpha[2 * k + 1]) || !std::isfinite(beta[2 * k]) || !std::isfinite(beta[2 * k + 1]))
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": omega^2 or omega times a damping coefficient overflows");
    }
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const int          kmax = std::min(n_freq, HARMONIC_CHUNK), nrow = h->NP * h->cfg.spacedim;
  const LodShape     wmax = lod_shape(h, kmax * n_rhs);
  const size_t       nvec = (size_t)nrow * kmax * n_rhs, npart = (size_t)wmax.ngroup * kmax * n_rhs;
  SlodDevBuf<double> work; // four products, two sets of partials, the norms of the chunk's columns
  hipError_t         e = work.alloc(4 * nvec + 2 * npart + (size_t)kmax * n_rhs);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who.c_str());
  double *au_re = work.get(), *au_im = au_re + nvec, *mu_re = au_im + nvec, *mu_im = mu_re + nvec;
  double *partial = mu_im + nvec, *partial_b = partial + npart, *d_norms = partial_b + npart;
  std::vector<double> norms((size_t)kmax * n_rhs);
  for (int k0 = 0; k0 < n_freq; k0 += HARMONIC_CHUNK)
    {
      const int        kc = std::min(HARMONIC_CHUNK, n_freq - k0), ncol = kc * n_rhs;
      const LodShape   w = lod_shape(h, ncol);
      SlodZFactorBuild z; // freed at the end of the chunk, after its wait
      if (const int rc = slod_lod_zfactor_launch(h, st, who.c_str(), d_stiffness, d_mass, d_cols, alpha.data() + 2 * k0,
                                                 beta.data() + 2 * k0, kc, &z))
        return rc;
      double *ur = d_u_re + (size_t)k0 * n_rhs, *ui = d_u_im + (size_t)k0 * n_rhs;
      slod_lod_zfactor_solve_launch(&z.f, st, 0, kc, d_load_re, d_load_im, ld_load, n_rhs, true, ur, ui, ld_u);
      slod_lod_apply_launch(h, st, d_stiffness, d_cols, ur, ld_u, ncol, au_re, (size_t)ncol);
      slod_lod_apply_launch(h, st, d_stiffness, d_cols, ui, ld_u, ncol, au_im, (size_t)ncol);
      slod_lod_apply_launch(h, st, d_mass, d_cols, ur, ld_u, ncol, mu_re, (size_t)ncol);
      slod_lod_apply_launch(h, st, d_mass, d_cols, ui, ld_u, ncol, mu_im, (size_t)ncol);
      hipLaunchKernelGGL(k_harmonic_residual, lod_grid(w, 1024), dim3(LOD_BLOCK), 0, st, nrow, n_rhs, ncol, w.ngroup, z.f.coef, au_re,
                         au_im, mu_re, mu_im, d_load_re, d_load_im, ld_load, partial, partial_b);
      hipLaunchKernelGGL(k_harmonic_norms, lod_flat_grid((size_t)ncol), dim3(LOD_BLOCK), 0, st, ncol, w.ngroup, partial, partial_b,
                         d_norms);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(norms.data(), d_norms, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st);
      // the one wait of the chunk, on every path: z and work are freed behind it
      const int rc = slod_lod_zfactor_finish(h, st, who.c_str(), "frequency", k0, &z, nullptr);
      if (e != hipSuccess)
        return slod_hip_fail(h, e, who.c_str());
      if (rc)
        return rc;
      if (rel_residual)
        std::copy(norms.begin(), norms.begin() + ncol, rel_residual + (size_t)k0 * n_rhs);
      if (growth)
        for (int k = 0; k < kc; ++k)
          growth[k0 + k] = z.f.inertia[(size_t)k].norm_factor / z.f.inertia[(size_t)k].norm_matrix;
    }
  return SLOD_OK;
}
#pragma GCC visibility pop
