// The frequency response on the LOD space: for  M u'' + C u' + A u = Re(b e^{i omega t}),  C = damp_mass M + damp_stiff A
// (the Rayleigh damping of the Newmark calls), the amplitude solves the complex symmetric system
//   S(omega) u = b,   S(omega) = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M.
//   slod_lod_harmonic_response   a sweep of frequencies in one call: frequency k is member k of a complex banded LDL^T
//                                (slod_lod_factor_create_zldl, slod_lod_factor.hip) with alpha_k = (1, omega_k damp_stiff),
//                                beta_k = (-(omega_k omega_k), omega_k damp_mass), solved on the shared load; then the true
//                                residual from the matrices themselves and the growth of every factor
//   slod_lod_harmonic_response_ensemble   the sweep for the K members of a coefficient ensemble on one pattern: the flat
//                                factor member j = k K + m is frequency k on the matrices of member m, solved on member m's
//                                load columns; u, rel_residual and growth of every (k, m) have the bits of the single call
//                                on member m at omega_k.  The chunks are runs of at most HARMONIC_CHUNK consecutive j.
// The sweep runs in chunks of at most HARMONIC_CHUNK frequencies (one factor allocation each), every chunk queued whole on
// the handle's stream and waited for once.  A member's bits do not depend on the members beside it, so the result does
// not depend on the chunking.
// Residual: the four products A u_re, A u_im, M u_re, M u_im by the fma chain of slod_lod_apply_multi, combined per entry
// with the complex coefficients (k_harmonic_residual: every product and sum rounded on its own, in one order), squared and
// summed over the rows of a group, then over the groups, both ascending (slod_lod_tile.hip.h): no atomics.
// The ensemble call forms the four products in one launch of k_harmonic_apply (the fma chain of slod_lod_apply_multi on
// the matrices of the column's member) and adds per row the parts of u^H M u, u^H A u and u^H b, summed the same way.
//   slod_lod_harmonic_response_damped   the single sweep with a third damping matrix D (a sponge layer):
//                                S(omega) gains i omega D, the factor is that of slod_lod_factor_create_zldl3 with
//                                gamma_k = (0, omega_k), the residual takes six products (k_harmonic_apply with the third
//                                matrix, one launch) and the quantities are five: u^H D u joins them.  Without D the sweep has
//                                the words of slod_lod_harmonic_response.
#include "slod_lod_tile.hip.h"

#include <cmath>
#include <vector>

namespace
{
  constexpr int HARMONIC_CHUNK = 64; // factor members (frequencies, or frequencies x ensemble members) per factor allocation

  // out[z][i][col] of the four products z = (A u_re, A u_im, M u_re, M u_im), plane doubles apart, for the chunk's column
  // (six with gridDim.z = 6: D u_re and D u_im of the third matrix d3, ld_d, follow)
  // col = k n_rhs + c: factor member k of the chunk reads the matrices of ensemble member (m0 + k) % kmat, entry e at
  // a[e ld_a + member].  The chain of slod_lod_apply_multi per (row, column) on those operands; grid as k_ens_apply, z: the
  // product.
  __global__ __launch_bounds__(LOD_BLOCK) void k_harmonic_apply(int nrow, int s, int cap, int NP, int n_rhs, int ncol, int ngroup, int kmat,
                                                              int m0, const double *__restrict__ a, size_t ld_a,
                                                              const double *__restrict__ m, size_t ld_m,
                                                              const double *__restrict__ d3, size_t ld_d,
                                                              const uint32_t *__restrict__ cols, const double *__restrict__ u_re,
                                                              const double *__restrict__ u_im, size_t ld_u, double *__restrict__ out,
                                                              size_t plane)
  {
    const double *values = blockIdx.z < 2 ? a : blockIdx.z < 4 ? m : d3, *x = (blockIdx.z & 1) ? u_im : u_re;
    const size_t  ld_v = blockIdx.z < 2 ? ld_a : blockIdx.z < 4 ? ld_m : ld_d;
    double       *y = out + blockIdx.z * plane;
    const int     c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, ncol - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
        {
          const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
          if (i >= nrow)
            continue;
          const int p = i / s, d = i - p * s, member = (m0 + col / n_rhs) % kmat;
          y[(size_t)i * ncol + col] = s == 1 ? slod_lod_row_product_per_col<1>(p, d, cap, NP, values, ld_v, cols, x, ld_u, col, member)
                                             : slod_lod_row_product_per_col<2>(p, d, cap, NP, values, ld_v, cols, x, ld_u, col, member);
        }
  }

  // partial[g][col] = sum over the rows of group g of |r|^2, r = b - ((alpha A + beta M) u) of column col = k n_rhs + c
  // (factor member k of the chunk, load column c);  partial_b[g][col] the same of |b|^2.  coef: [members][4] of the factor.
  // Member k reads the load columns ((m0 + k) % kmat) n_rhs + c: kmat = 1 is the load shared by all frequencies.
  // QUANT: partial_q[q][g][col], npart doubles apart, the same sums of the four parts per row
  //   u_re (M u)_re + u_im (M u)_im,   u_re (A u)_re + u_im (A u)_im,   u_re b_re + u_im b_im,   u_re b_im - u_im b_re
  // (u^H M u, u^H A u, Re u^H b, Im u^H b), every product and sum rounded on its own; u: the chunk's columns.
  // THREE: S u = (alpha (A u) + beta (M u)) + gamma (D u) with the products du_re, du_im and coef_c: [members][2]; with QUANT
  // the parts are five, u_re (D u)_re + u_im (D u)_im (u^H D u) third: (M, A, D, Re u^H b, Im u^H b).
  template <bool QUANT, bool THREE = false>
  __global__ __launch_bounds__(LOD_BLOCK) void k_harmonic_residual(int nrow, int n_rhs, int ncol, int ngroup, int kmat, int m0,
                                                                 const double *__restrict__ coef, const double *__restrict__ au_re,
                                                                 const double *__restrict__ au_im, const double *__restrict__ mu_re,
                                                                 const double *__restrict__ mu_im, const double *__restrict__ du_re,
                                                                 const double *__restrict__ du_im, const double *__restrict__ coef_c,
                                                                 const double *__restrict__ b_re,
                                                                 const double *__restrict__ b_im, size_t ld_b,
                                                                 const double *__restrict__ u_re, const double *__restrict__ u_im,
                                                                 size_t ld_u, double *__restrict__ partial,
                                                                 double *__restrict__ partial_b, double *__restrict__ partial_q,
                                                                 size_t npart)
  {
#pragma clang fp contract(off)
    __shared__ double sR[LOD_ROWS][LOD_COLS], sB[LOD_ROWS][LOD_COLS];
    constexpr int NQ = QUANT ? (THREE ? 5 : 4) : 1, QB = THREE ? 3 : 2; // QB: where the two parts of u^H b stand
    __shared__ double sQ[NQ][LOD_ROWS][LOD_COLS];
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, ncol - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
          {
            const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
            double    rr = 0.0, bb = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, qd = 0.0;
            if (i < nrow)
              {
                const int     k = col / n_rhs, lc = ((m0 + k) % kmat) * n_rhs + (col - k * n_rhs);
                const double *ck = coef + 4 * k;
                const size_t  at = (size_t)i * ncol + col;
                const double  ar = au_re[at], ai = au_im[at], mr = mu_re[at], mi = mu_im[at];
                const double  br = b_re[(size_t)i * ld_b + lc], bi = b_im ? b_im[(size_t)i * ld_b + lc] : 0.0;
                double        dr = 0.0, di = 0.0;
                if constexpr (THREE)
                  dr = du_re[at], di = du_im[at];
                if constexpr (QUANT)
                  {
                    const double ur = u_re[(size_t)i * ld_u + col], ui = u_im[(size_t)i * ld_u + col];
                    if constexpr (THREE)
                      qd = ur * dr + ui * di;
                    q0 = ur * mr + ui * mi;
                    q1 = ur * ar + ui * ai;
                    q2 = ur * br + ui * bi;
                    q3 = ur * bi - ui * br;
                  }
                // S u = alpha (A u) + beta (M u), complex products written out
                double sr = ((ck[0] * ar - ck[1] * ai) + (ck[2] * mr - ck[3] * mi));
                double si = ((ck[0] * ai + ck[1] * ar) + (ck[2] * mi + ck[3] * mr));
                if constexpr (THREE)
                  {
                    const double *gk = coef_c + 2 * k;
                    sr = sr + (gk[0] * dr - gk[1] * di);
                    si = si + (gk[0] * di + gk[1] * dr);
                  }
                const double er = br - sr, ei = bi - si;
                rr = er * er + ei * ei;
                bb = br * br + bi * bi;
              }
            sR[lr][c] = rr, sB[lr][c] = bb;
            if constexpr (QUANT)
              {
                sQ[0][lr][c] = q0, sQ[1][lr][c] = q1, sQ[QB][lr][c] = q2, sQ[QB + 1][lr][c] = q3;
                if constexpr (THREE)
                  sQ[2][lr][c] = qd;
              }
          }
        __syncthreads();
        if ((int)threadIdx.x < nb)
          {
            partial[(size_t)g * ncol + c0 + threadIdx.x]   = slod_lod_group_sum(sR, threadIdx.x);
            partial_b[(size_t)g * ncol + c0 + threadIdx.x] = slod_lod_group_sum(sB, threadIdx.x);
            if constexpr (QUANT)
              for (int q = 0; q < NQ; ++q)
                partial_q[q * npart + (size_t)g * ncol + c0 + threadIdx.x] = slod_lod_group_sum(sQ[q], threadIdx.x);
          }
        __syncthreads();
      }
  }

  // out[col] = ||r||_2 / ||b||_2, the groups summed in ascending order; a zero load column gives 0.
  // NQ > 0: out[ncol + NQ col + q] the NQ (four, with a third matrix five) sums of partial_q over the groups, ascending.
  template <int NQ>
  __global__ __launch_bounds__(LOD_BLOCK) void k_harmonic_norms(int ncol, int ngroup, const double *__restrict__ partial,
                                                              const double *__restrict__ partial_b,
                                                              const double *__restrict__ partial_q, size_t npart,
                                                              double *__restrict__ out)
  {
    const int col = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (col >= ncol)
      return;
    const double rr = slod_lod_ordered_sum(partial, ngroup, ncol, col), bb = slod_lod_ordered_sum(partial_b, ngroup, ncol, col);
    out[col] = bb > 0.0 ? sqrt(rr) / sqrt(bb) : (rr > 0.0 ? HUGE_VAL : 0.0);
    for (int q = 0; q < NQ; ++q)
      out[ncol + NQ * col + q] = slod_lod_ordered_sum(partial_q + q * npart, ngroup, ncol, col);
  }

  // what both calls refuse about the sweep itself, and the coefficients alpha_k = (1, omega_k damp_stiff),
  // beta_k = (-(omega_k omega_k), omega_k damp_mass), one rounding per part
  int harmonic_coefficients(slod_handle *h, const std::string &who, double damp_mass, double damp_stiff, const double *omega, int n_freq,
                            int n_rhs, std::vector<double> &alpha, std::vector<double> &beta)
  {
    if (!(damp_mass >= 0.0) || !(damp_stiff >= 0.0) || std::isinf(damp_mass) || std::isinf(damp_stiff))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": negative, NaN or infinite damping coefficient");
    if (n_freq < 1 || n_rhs < 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_freq < 1 or n_rhs < 1");
    for (int k = 0; k < n_freq; ++k)
      if (!(omega[k] >= 0.0) || std::isinf(omega[k]))
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": a frequency is negative, NaN or infinite");
    // (-(omega omega), omega damp) must be finite for the factor
    alpha.resize(2 * (size_t)n_freq), beta.resize(2 * (size_t)n_freq);
    for (int k = 0; k < n_freq; ++k)
      {
        const double w = omega[k];
        alpha[2 * k] = 1.0, alpha[2 * k + 1] = w * damp_stiff;
        beta[2 * k] = -(w * w), beta[2 * k + 1] = w * damp_mass;
        if (!std::isfinite(alpha[2 * k + 1]) || !std::isfinite(beta[2 * k]) || !std::isfinite(beta[2 * k + 1]))
          return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": omega^2 or omega times a damping coefficient overflows");
      }
    return SLOD_OK;
  }
} // namespace

namespace
{
  // The sweep on one matrix pair, the body of slod_lod_harmonic_response and of slod_lod_harmonic_response_damped.  The
  // first (damped unset) queues per chunk the factor, the solve, four products by slod_lod_apply_multi's launch and the
  // residual.  The second forms the products in one launch of k_harmonic_apply (the same chains) and the quantities with
  // the residual; with d_damping the factor, the residual and the quantities take the third matrix.  quantities: HOST
  // [n_freq n_rhs][5], may be NULL.
  int harmonic_single(slod_handle *h, const std::string &who, bool damped, const double *d_stiffness, const double *d_mass,
                      const double *d_damping, const uint32_t *d_cols, double damp_mass, double damp_stiff, const double *omega,
                      int n_freq, const double *d_load_re, const double *d_load_im, size_t ld_load, int n_rhs, double *d_u_re,
                      double *d_u_im, size_t ld_u, double *rel_residual, double *growth, double *quantities)
  {
    if (!h || !d_stiffness || !d_mass || !d_cols || !omega || !d_load_re || !d_u_re || !d_u_im)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL handle, matrix, d_cols, omega, load or u");
    std::vector<double> alpha, beta, gamma;
    if (const int rc = harmonic_coefficients(h, who, damp_mass, damp_stiff, omega, n_freq, n_rhs, alpha, beta))
      return rc;
    if (ld_load < (size_t)n_rhs)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of the load below n_rhs");
    if (ld_u / (size_t)n_rhs < (size_t)n_freq)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of u below n_freq * n_rhs");
    const bool three = d_damping != nullptr;
    if (three) // gamma_k = (0, omega_k)
      {
        gamma.assign(2 * (size_t)n_freq, 0.0);
        for (int k = 0; k < n_freq; ++k)
          gamma[2 * k + 1] = omega[k];
      }
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const int          kmax = std::min(n_freq, HARMONIC_CHUNK), nrow = h->NP * h->cfg.spacedim, nq = !damped ? 0 : three ? 5 : 4;
    const int          nprod = three ? 6 : 4;
    const LodShape     wmax = lod_shape(h, kmax * n_rhs);
    const size_t       nvec = (size_t)nrow * kmax * n_rhs, npart = (size_t)wmax.ngroup * kmax * n_rhs;
    SlodDevBuf<double> work; // the products, two sets of partials and those of the quantities, the norms and quantities of the chunk
    hipError_t         e = work.alloc(nprod * nvec + (2 + nq) * npart + (1 + nq) * (size_t)kmax * n_rhs);
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who.c_str());
    double *prod = work.get(), *partial = prod + nprod * nvec, *partial_b = partial + npart, *partial_q = partial_b + npart;
    double *d_norms = partial_q + nq * npart;
    std::vector<double> norms((1 + nq) * (size_t)kmax * n_rhs);
    for (int k0 = 0; k0 < n_freq; k0 += HARMONIC_CHUNK)
      {
        const int        kc = std::min(HARMONIC_CHUNK, n_freq - k0), ncol = kc * n_rhs;
        const LodShape   w = lod_shape(h, ncol);
        const size_t     plane = damped ? (size_t)nrow * ncol : nvec;
        double          *au_re = prod, *au_im = prod + plane, *mu_re = prod + 2 * plane, *mu_im = prod + 3 * plane;
        SlodZFactorBuild z; // freed at the end of the chunk, after its wait
        if (const int rc = slod_lod_zfactor_launch(h, st, who.c_str(), d_stiffness, 1, d_mass, 1, 1, d_cols, alpha.data(), beta.data(),
                                                   (size_t)k0, kc, &z, d_damping, 1, three ? gamma.data() : nullptr))
          return rc;
        double *ur = d_u_re + (size_t)k0 * n_rhs, *ui = d_u_im + (size_t)k0 * n_rhs;
        slod_lod_zfactor_solve_launch(&z.f, st, 0, kc, d_load_re, d_load_im, ld_load, n_rhs, 0, 1, ur, ui, ld_u);
        if (!damped)
          {
            slod_lod_apply_launch(h, st, d_stiffness, d_cols, ur, ld_u, ncol, au_re, (size_t)ncol);
            slod_lod_apply_launch(h, st, d_stiffness, d_cols, ui, ld_u, ncol, au_im, (size_t)ncol);
            slod_lod_apply_launch(h, st, d_mass, d_cols, ur, ld_u, ncol, mu_re, (size_t)ncol);
            slod_lod_apply_launch(h, st, d_mass, d_cols, ui, ld_u, ncol, mu_im, (size_t)ncol);
            hipLaunchKernelGGL(k_harmonic_residual<false>, lod_grid(w, 1024), dim3(LOD_BLOCK), 0, st, nrow, n_rhs, ncol, w.ngroup, 1, 0,
                               z.f.coef, au_re, au_im, mu_re, mu_im, nullptr, nullptr, nullptr, d_load_re, d_load_im, ld_load, nullptr,
                               nullptr, 0, partial, partial_b, nullptr, 0);
            hipLaunchKernelGGL(k_harmonic_norms<0>, lod_flat_grid((size_t)ncol), dim3(LOD_BLOCK), 0, st, ncol, w.ngroup, partial,
                               partial_b, nullptr, 0, d_norms);
          }
        else
          {
            hipLaunchKernelGGL(k_harmonic_apply, lod_grid(w, 1024, nprod), dim3(LOD_BLOCK), 0, st, nrow, w.s, w.cap, w.NP, n_rhs, ncol,
                               w.ngroup, 1, 0, d_stiffness, 1, d_mass, 1, d_damping, 1, d_cols, ur, ui, ld_u, prod, plane);
            const auto residual = three ? k_harmonic_residual<true, true> : k_harmonic_residual<true, false>;
            hipLaunchKernelGGL(residual, lod_grid(w, 1024), dim3(LOD_BLOCK), 0, st, nrow, n_rhs, ncol, w.ngroup, 1, 0, z.f.coef, au_re, au_im, mu_re, mu_im,
                               prod + 4 * plane, prod + 5 * plane, three ? z.f.coef + 4 * (size_t)kc : nullptr, d_load_re, d_load_im, ld_load, ur, ui,
                               ld_u, partial, partial_b, partial_q, npart);
            hipLaunchKernelGGL(three ? k_harmonic_norms<5> : k_harmonic_norms<4>, lod_flat_grid((size_t)ncol), dim3(LOD_BLOCK), 0, st,
                               ncol, w.ngroup, partial, partial_b, partial_q, npart, d_norms);
          }
        e = hipGetLastError();
        if (e == hipSuccess)
          e = hipMemcpyAsync(norms.data(), d_norms, (1 + nq) * (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st);
        // the one wait of the chunk, on every path: z and work are freed behind it
        const int rc = slod_lod_zfactor_finish(h, st, who.c_str(), "frequency", (size_t)k0, &z, nullptr);
        if (e != hipSuccess)
          return slod_hip_fail(h, e, who.c_str());
        if (rc)
          return rc;
        if (rel_residual)
          std::copy(norms.begin(), norms.begin() + ncol, rel_residual + (size_t)k0 * n_rhs);
        if (quantities) // (u^H M u, u^H A u, u^H D u, Re u^H b, Im u^H b); without D the third is +0.0
          for (int c = 0; c < ncol; ++c)
            {
              const double *q = norms.data() + ncol + (size_t)nq * c;
              double       *out = quantities + 5 * ((size_t)k0 * n_rhs + c);
              out[0] = q[0], out[1] = q[1], out[2] = three ? q[2] : 0.0, out[3] = q[nq - 2], out[4] = q[nq - 1];
            }
        if (growth)
          for (int k = 0; k < kc; ++k)
            growth[k0 + k] = z.f.inertia[(size_t)k].norm_factor / z.f.inertia[(size_t)k].norm_matrix;
      }
    return SLOD_OK;
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" int slod_lod_harmonic_response(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                                          double damp_mass, double damp_stiff, const double *omega, int n_freq, const double *d_load_re,
                                          const double *d_load_im, size_t ld_load, int n_rhs, double *d_u_re, double *d_u_im,
                                          size_t ld_u, double *rel_residual, double *growth)
{
  return harmonic_single(h, "slod_lod_harmonic_response", false, d_stiffness, d_mass, nullptr, d_cols, damp_mass, damp_stiff, omega,
                         n_freq, d_load_re, d_load_im, ld_load, n_rhs, d_u_re, d_u_im, ld_u, rel_residual, growth, nullptr);
}

extern "C" int slod_lod_harmonic_response_damped(slod_handle *h, const double *d_stiffness, const double *d_mass,
                                                 const double *d_damping, const uint32_t *d_cols, double damp_mass, double damp_stiff,
                                                 const double *omega, int n_freq, const double *d_load_re, const double *d_load_im,
                                                 size_t ld_load, int n_rhs, double *d_u_re, double *d_u_im, size_t ld_u,
                                                 double *rel_residual, double *growth, double *quantities)
{
  return harmonic_single(h, "slod_lod_harmonic_response_damped", true, d_stiffness, d_mass, d_damping, d_cols, damp_mass, damp_stiff,
                         omega, n_freq, d_load_re, d_load_im, ld_load, n_rhs, d_u_re, d_u_im, ld_u, rel_residual, growth, quantities);
}

extern "C" int slod_lod_harmonic_response_ensemble(slod_handle *h, const double *d_stiffness, size_t ld_a_m, const double *d_mass,
                                                   size_t ld_m_m, const uint32_t *d_cols, int n_members, double damp_mass,
                                                   double damp_stiff, const double *omega, int n_freq, const double *d_load_re,
                                                   const double *d_load_im, size_t ld_load, int n_rhs, double *d_u_re, double *d_u_im,
                                                   size_t ld_u, double *rel_residual, double *growth, double *quantities)
{
  const std::string who = "slod_lod_harmonic_response_ensemble";
  if (!h || !d_stiffness || !d_mass || !d_cols || !omega || !d_load_re || !d_u_re || !d_u_im)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL handle, matrix, d_cols, omega, load or u");
  if (n_members < 1 || n_members > 65535)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_members < 1 or > 65535");
  std::vector<double> alpha, beta;
  if (const int rc = harmonic_coefficients(h, who, damp_mass, damp_stiff, omega, n_freq, n_rhs, alpha, beta))
    return rc;
  if (ld_a_m < (size_t)n_members || ld_m_m < (size_t)n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of a matrix below n_members");
  if (ld_load / (size_t)n_rhs < (size_t)n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of the load below n_members * n_rhs");
  const size_t K = (size_t)n_members, total = (size_t)n_freq * K; // flat factor members j = k K + m
  if (ld_u / (size_t)n_rhs < total)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": leading dimension of u below n_freq * n_members * n_rhs");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const int          jmax = (int)std::min(total, (size_t)HARMONIC_CHUNK), nrow = h->NP * h->cfg.spacedim;
  const LodShape     wmax = lod_shape(h, jmax * n_rhs);
  const size_t       nvec = (size_t)nrow * jmax * n_rhs, npart = (size_t)wmax.ngroup * jmax * n_rhs;
  SlodDevBuf<double> work; // four products, six sets of partials, the norms and the four quantities of the chunk's columns
  hipError_t         e = work.alloc(4 * nvec + 6 * npart + 5 * (size_t)jmax * n_rhs);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who.c_str());
  double *prod = work.get(), *partial = prod + 4 * nvec, *partial_b = partial + npart, *partial_q = partial_b + npart;
  double *d_norms = partial_q + 4 * npart;
  std::vector<double> norms(5 * (size_t)jmax * n_rhs);
  for (size_t j0 = 0; j0 < total; j0 += HARMONIC_CHUNK)
    {
      const int        jc = (int)std::min((size_t)HARMONIC_CHUNK, total - j0), ncol = jc * n_rhs, m0 = (int)(j0 % K);
      const LodShape   w = lod_shape(h, ncol);
      const size_t     plane = (size_t)nrow * ncol;
      SlodZFactorBuild z; // freed at the end of the chunk, after its wait
      if (const int rc = slod_lod_zfactor_launch(h, st, who.c_str(), d_stiffness, ld_a_m, d_mass, ld_m_m, n_members, d_cols,
                                                 alpha.data(), beta.data(), j0, jc, &z))
        return rc;
      double *ur = d_u_re + j0 * n_rhs, *ui = d_u_im + j0 * n_rhs;
      slod_lod_zfactor_solve_launch(&z.f, st, 0, jc, d_load_re, d_load_im, ld_load, n_rhs, m0, n_members, ur, ui, ld_u);
      hipLaunchKernelGGL(k_harmonic_apply, lod_grid(w, 1024, 4), dim3(LOD_BLOCK), 0, st, nrow, w.s, w.cap, w.NP, n_rhs, ncol, w.ngroup,
                         n_members, m0, d_stiffness, ld_a_m, d_mass, ld_m_m, nullptr, 1, d_cols, ur, ui, ld_u, prod, plane);
      hipLaunchKernelGGL(k_harmonic_residual<true>, lod_grid(w, 1024), dim3(LOD_BLOCK), 0, st, nrow, n_rhs, ncol, w.ngroup, n_members,
                         m0, z.f.coef, prod, prod + plane, prod + 2 * plane, prod + 3 * plane, nullptr, nullptr, nullptr, d_load_re,
                         d_load_im, ld_load, ur, ui,
                         ld_u, partial, partial_b, partial_q, npart);
      hipLaunchKernelGGL(k_harmonic_norms<4>, lod_flat_grid((size_t)ncol), dim3(LOD_BLOCK), 0, st, ncol, w.ngroup, partial,
                         partial_b, partial_q, npart, d_norms);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(norms.data(), d_norms, 5 * (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st);
      // the one wait of the chunk, on every path: z and work are freed behind it
      const int rc = slod_lod_zfactor_finish(h, st, who.c_str(), "frequency", j0, &z, nullptr, "member", n_members);
      if (e != hipSuccess)
        return slod_hip_fail(h, e, who.c_str());
      if (rc)
        return rc;
      if (rel_residual)
        std::copy(norms.begin(), norms.begin() + ncol, rel_residual + j0 * n_rhs);
      if (quantities)
        std::copy(norms.begin() + ncol, norms.begin() + 5 * (size_t)ncol, quantities + 4 * j0 * n_rhs);
      if (growth)
        for (int k = 0; k < jc; ++k)
          growth[j0 + k] = z.f.inertia[(size_t)k].norm_factor / z.f.inertia[(size_t)k].norm_matrix;
    }
  return SLOD_OK;
}
#pragma GCC visibility pop
