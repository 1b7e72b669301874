// The LOD systems of a coefficient ensemble in one call each (the reference solves one problem, LOD.cc:976-1002): the K
// members of a handle with n_problems = K share the grid, hence the pattern of A_LOD, and differ in every value.  The
// matrices are stored member-minor on the one pattern (include/slod.h, "ensemble matrix"), so that member k is column k
// of the coarse multi-vectors and the tiling of slod_lod_tile.hip.h (columns on lanes) serves unchanged: where the
// shared-matrix product has all lanes of a wave read one word, here they read 64 consecutive ones.
//
// Nothing is summed in a new order.  Matrix, load and reconstruction run the bodies of slod_lod_system.hip.h with the
// member on blockIdx.y; the product is slod_lod_row_product<true>; the solve is SlodLodWork::solve with a matrix per
// column (slod_lod_multi.hip).  Every member's result has the bits of the single-problem call on its slab.
// The L2 side (mass matrix, symmetrised stiffness, combinations) follows the same rule: the row of k_lod_mass and the
// words of k_lod_symmetrize and k_lod_combine (slod_lod_system.hip.h) with the member on a grid axis or on the fastest
// thread index.
#include "slod_lod_system.hip.h"
#include "slod_lod_tile.hip.h"

namespace
{
  constexpr int    APPLY_MAX_BLOCKS = 1024;  // blocks per chunk, as k_lod_apply
  constexpr size_t MAX_MEMBERS      = 65535; // members sit on blockIdx.y

  // block = (row patch blockIdx.x, member blockIdx.y); the columns are the same for every member: member 0 writes them
  __global__ __launch_bounds__(256) void k_ens_matrix(const SlodGrid G, const double *basis, const double *premult, size_t stride,
                                                     size_t member_stride, double *values, size_t ld_m, uint32_t *cols)
  {
    const size_t k = blockIdx.y;
    lod_matrix_row(G, blockIdx.x, blockIdx.x, basis + k * member_stride, premult + k * member_stride, stride, values + k, ld_m,
                   k == 0 ? cols : nullptr);
  }

  // the row of k_lod_mass (slod_lod_time.hip); ld_rho = 0: one density for all members, rho NULL: density 1
  template <int S>
  __global__ __launch_bounds__(256) void k_ens_mass(const SlodGrid G, const double *basis, size_t stride, size_t member_stride,
                                                   const double *rho, size_t ld_rho, double scale, double *values, size_t ld_m,
                                                   uint32_t *cols)
  {
    const size_t k = blockIdx.y;
    lod_mass_row<S>(G, blockIdx.x, blockIdx.x, basis + k * member_stride, stride, rho ? rho + k * ld_rho : nullptr, scale,
                    values + k, ld_m, k == 0 ? cols : nullptr);
  }

  // one thread per (word w, member k), k fastest: the lanes of a wave read consecutive doubles
  __global__ __launch_bounds__(256) void k_ens_symmetrize(int NP, int s, int cap, int n_members, const double *__restrict__ values,
                                                         size_t ld_in, const uint32_t *__restrict__ cols, double *__restrict__ out,
                                                         size_t ld_out)
  {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, w = t / n_members, k = t - w * n_members;
    if (w < (size_t)NP * cap * s * s)
      out[w * ld_out + k] = lod_symmetrize_word(NP, s, cap, values + k, ld_in, cols, w);
  }

  // a, b and out may be one array when their leading dimensions agree: a thread reads its two words, then writes its own
  __global__ __launch_bounds__(256) void k_ens_combine(size_t n, int n_members, double alpha, const double *a, size_t ld_a,
                                                      double beta, const double *b, size_t ld_b, double *out, size_t ld_out)
  {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, w = t / n_members, k = t - w * n_members;
    if (w < n)
      out[w * ld_out + k] = lod_combine_word(alpha, a[w * ld_a + k], beta, b[w * ld_b + k]);
  }

  // ld_fine = 0: one load for all members
  __global__ __launch_bounds__(256) void k_ens_rhs(const SlodGrid G, const double *basis, size_t stride, size_t member_stride,
                                                  const double *frhs, size_t ld_fine, double *out, size_t ld_out)
  {
    const size_t k = blockIdx.y;
    lod_rhs_row(G, blockIdx.x, blockIdx.x, basis + k * member_stride, stride, frhs + k * ld_fine, out + k, ld_out);
  }

  // one thread per (global fine node, member)
  __global__ __launch_bounds__(256) void k_ens_reconstruct(const SlodGrid G, const double *basis, size_t stride,
                                                          size_t member_stride, const double *u, size_t ld_u, double *fine,
                                                          size_t ld_fine)
  {
    const size_t k   = blockIdx.y;
    const int    NEp = G.N * G.n_sub + 1, gn = blockIdx.x * 256 + threadIdx.x;
    if (gn < NEp * NEp)
      lod_reconstruct_node(G, gn, basis + k * member_stride, stride, u + k, ld_u, fine + k * ld_fine);
  }

  // Y_k = A_k X_k: the tiling of k_lod_apply (slod_lod_time.hip), the row product with a matrix per column
  __global__ __launch_bounds__(LOD_BLOCK) void k_ens_apply(int nrow, int s, int cap, int NP, int n_members, int ngroup,
                                                          const double *__restrict__ values, size_t ld_m,
                                                          const uint32_t *__restrict__ cols, const double *__restrict__ x,
                                                          size_t ld_x, double *__restrict__ y, size_t ld_y)
  {
    const int c0 = blockIdx.y * LOD_COLS, nb = min(LOD_COLS, n_members - c0);
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      for (int idx = threadIdx.x; idx < LOD_ROWS * nb; idx += LOD_BLOCK)
        {
          const int lr = idx / nb, c = idx - lr * nb, i = g * LOD_ROWS + lr, col = c0 + c;
          if (i >= nrow)
            continue;
          const double acc = slod_lod_row_product<true>(i, s, cap, NP, values, cols, x, ld_x, col, ld_m);
          y[(size_t)i * ld_y + col] = acc;
        }
  }

  // Mean and unbiased variance over the members, one thread per entry (reads coalesced along i), members ascending;
  // difference, product and sums rounded on their own.  The second loop reads what the first just brought in.
  __global__ __launch_bounds__(256) void k_ens_moments(const double *fields, size_t ld_fine, int n_members, size_t count,
                                                      double *mean, double *var)
  {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count)
      return;
    double sum = fields[i];
    for (int k = 1; k < n_members; ++k)
      sum = sum + fields[(size_t)k * ld_fine + i];
    const double m = sum / (double)n_members;
    mean[i]        = m;
    if (!var)
      return;
    double acc = 0.0;
    for (int k = 0; k < n_members; ++k)
      {
        const double d = fields[(size_t)k * ld_fine + i] - m, d2 = d * d;
        acc            = acc + d2;
      }
    var[i] = n_members > 1 ? acc / (double)(n_members - 1) : 0.0;
  }

  // The checks every call on n_members members shares; lds: the leading dimensions that hold a member per column
  int ens_check(const slod_handle *h, const char *who, bool arrays, int n_members, std::initializer_list<size_t> lds)
  {
    if (!h || !arrays)
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
    if (n_members < 1 || (size_t)n_members > MAX_MEMBERS)
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or > 65535");
    return slod_check_ld(h, who, "n_members", n_members, lds);
  }
  // member_stride must hold a slab of num_patches * stride doubles as soon as there is a second member
  int ens_check_slab(const slod_handle *h, const char *who, size_t stride, size_t member_stride, int n_members)
  {
    if (n_members > 1 && member_stride < (size_t)h->NP * stride)
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": member_stride shorter than a slab");
    return SLOD_OK;
  }
  size_t ens_field(const slod_handle *h) { return (size_t)(h->NE + 1) * (h->NE + 1) * h->cfg.spacedim; }
  size_t ens_words(const slod_handle *h)
  {
    const size_t s = (size_t)h->cfg.spacedim;
    return (size_t)h->NP * slod_lod_row_capacity(h) * s * s;
  }
} // namespace

// k_ens_apply for the time loop on an ensemble factor (slod_lod_time.hip); arguments are checked by the caller
void slod_lod_apply_ensemble_launch(const slod_handle *h, hipStream_t st, const double *d_values, size_t ld_m, const uint32_t *d_cols,
                                    const double *d_x, size_t ld_x, int n_members, double *d_y, size_t ld_y)
{
  const LodShape w = lod_shape(h, n_members);
  hipLaunchKernelGGL(k_ens_apply, lod_grid(w, APPLY_MAX_BLOCKS), dim3(LOD_BLOCK), 0, st, w.nrow, w.s, w.cap, w.NP, n_members, w.ngroup,
                     d_values, ld_m, d_cols, d_x, ld_x, d_y, ld_y);
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_matrix_ensemble(slod_handle *h, const double *d_basis, const double *d_premult, size_t stride, size_t member_stride,
                             int n_members, double *d_values, size_t ld_m, uint32_t *d_cols, void *hip_stream)
{
  const char *who = "slod_lod_matrix_ensemble";
  if (const int rc = ens_check(h, who, d_basis && d_premult && d_values && d_cols, n_members, {ld_m}))
    return rc;
  if (const int rc = ens_check_slab(h, who, stride, member_stride, n_members))
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  hipLaunchKernelGGL(k_ens_matrix, dim3((unsigned)h->NP, (unsigned)n_members), dim3(256), 0, st, slod_grid_of(h), d_basis, d_premult,
                     stride, member_stride, d_values, ld_m, d_cols);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_mass_matrix_ensemble(slod_handle *h, const double *d_basis, size_t stride, size_t member_stride, int n_members,
                                  const double *d_rho, size_t ld_rho, double *d_values, size_t ld_m, uint32_t *d_cols, void *hip_stream)
{
  const char *who = "slod_lod_mass_matrix_ensemble";
  if (const int rc = ens_check(h, who, d_basis && d_values && d_cols, n_members, {ld_m}))
    return rc;
  if (const int rc = ens_check_slab(h, who, stride, member_stride, n_members))
    return rc;
  if (d_rho && ld_rho != 0 && ld_rho < (size_t)h->NE * h->NE)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": ld_rho not 0 and shorter than a density field");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const double hf = 1.0 / h->NE, scale = hf * hf / 36.0; // as slod_lod_mass_matrix
  const dim3   grid((unsigned)h->NP, (unsigned)n_members);
  if (h->cfg.spacedim == 1)
    hipLaunchKernelGGL(k_ens_mass<1>, grid, dim3(256), 0, st, slod_grid_of(h), d_basis, stride, member_stride, d_rho, ld_rho, scale,
                       d_values, ld_m, d_cols);
  else
    hipLaunchKernelGGL(k_ens_mass<2>, grid, dim3(256), 0, st, slod_grid_of(h), d_basis, stride, member_stride, d_rho, ld_rho, scale,
                       d_values, ld_m, d_cols);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_matrix_symmetrize_ensemble(slod_handle *h, const double *d_values, size_t ld_in, const uint32_t *d_cols, int n_members,
                                        double *d_out, size_t ld_out, void *hip_stream)
{
  const char *who = "slod_lod_matrix_symmetrize_ensemble";
  if (const int rc = ens_check(h, who, d_values && d_cols && d_out, n_members, {ld_in, ld_out}))
    return rc;
  if (d_out == d_values)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": a row reads other rows, the call cannot run in place");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const LodShape w = lod_shape(h, 1);
  hipLaunchKernelGGL(k_ens_symmetrize, lod_flat_grid(ens_words(h) * n_members), dim3(256), 0, st, w.NP, w.s, w.cap, n_members, d_values,
                     ld_in, d_cols, d_out, ld_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_matrix_combine_ensemble(slod_handle *h, double alpha, const double *d_a, size_t ld_a, double beta, const double *d_b,
                                     size_t ld_b, int n_members, double *d_out, size_t ld_out, void *hip_stream)
{
  const char *who = "slod_lod_matrix_combine_ensemble";
  if (const int rc = ens_check(h, who, d_a && d_b && d_out, n_members, {ld_a, ld_b, ld_out}))
    return rc;
  if ((d_out == d_a && ld_out != ld_a) || (d_out == d_b && ld_out != ld_b))
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": in place needs equal leading dimensions");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const size_t n = ens_words(h);
  hipLaunchKernelGGL(k_ens_combine, lod_flat_grid(n * n_members), dim3(256), 0, st, n, n_members, alpha, d_a, ld_a, beta, d_b, ld_b,
                     d_out, ld_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_rhs_ensemble(slod_handle *h, const double *d_basis, size_t stride, size_t member_stride, int n_members,
                          const double *d_fine_rhs, size_t ld_fine, double *d_out, size_t ld_out, void *hip_stream)
{
  const char *who = "slod_lod_rhs_ensemble";
  if (const int rc = ens_check(h, who, d_basis && d_fine_rhs && d_out, n_members, {ld_out}))
    return rc;
  if (const int rc = ens_check_slab(h, who, stride, member_stride, n_members))
    return rc;
  if (ld_fine != 0 && ld_fine < ens_field(h))
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": ld_fine not 0 and shorter than a fine field");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  hipLaunchKernelGGL(k_ens_rhs, dim3((unsigned)h->NP, (unsigned)n_members), dim3(256), 0, st, slod_grid_of(h), d_basis, stride,
                     member_stride, d_fine_rhs, ld_fine, d_out, ld_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_apply_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols, const double *d_x,
                            size_t ld_x, int n_members, double *d_y, size_t ld_y, void *hip_stream)
{
  const char *who = "slod_lod_apply_ensemble";
  if (const int rc = ens_check(h, who, d_values && d_cols && d_x && d_y, n_members, {ld_m, ld_x, ld_y}))
    return rc;
  if (d_x == d_y)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": the product cannot run in place");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  slod_lod_apply_ensemble_launch(h, st, d_values, ld_m, d_cols, d_x, ld_x, n_members, d_y, ld_y);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_solve_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols, const double *d_rhs,
                            size_t ld_rhs, int n_members, double *d_u, size_t ld_u, double rel_tol, int max_iterations,
                            int *iterations, double *rel_residual)
{
  const char *who = "slod_lod_solve_ensemble";
  if (const int rc = ens_check(h, who, d_values && d_cols && d_rhs && d_u, n_members, {ld_m, ld_rhs, ld_u}))
    return rc;
  if (max_iterations < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": max_iterations < 0");
  if (const int rc = slod_enter(h, nullptr, nullptr))
    return rc;
  // workspace allocated per call; the solve synchronises the stream before it returns
  SlodLodWork work;
  hipError_t  e = work.alloc(n_members, [&](SlodCarver &c) { work.take_solve(c, h, true); });
  if (e == hipSuccess)
    e = work.solve(h, d_values, d_cols, d_rhs, ld_rhs, d_u, ld_u, rel_tol, max_iterations, ld_m);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who);
  work.report(iterations, rel_residual);
  return work.last;
}

int slod_lod_reconstruct_ensemble(slod_handle *h, const double *d_basis, size_t stride, size_t member_stride, int n_members,
                                  const double *d_u, size_t ld_u, double *d_fine, size_t ld_fine, void *hip_stream)
{
  const char *who = "slod_lod_reconstruct_ensemble";
  if (const int rc = ens_check(h, who, d_basis && d_u && d_fine, n_members, {ld_u}))
    return rc;
  if (const int rc = ens_check_slab(h, who, stride, member_stride, n_members))
    return rc;
  if (ld_fine < ens_field(h))
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": ld_fine shorter than a fine field");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int NEp = h->NE + 1;
  hipLaunchKernelGGL(k_ens_reconstruct, dim3((unsigned)((NEp * NEp + 255) / 256), (unsigned)n_members), dim3(256), 0, st,
                     slod_grid_of(h), d_basis, stride, member_stride, d_u, ld_u, d_fine, ld_fine);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_ensemble_moments(slod_handle *h, const double *d_fields, size_t ld_fine, int n_members, size_t count, double *d_mean,
                          double *d_var, void *hip_stream)
{
  const char *who = "slod_ensemble_moments";
  if (!h || !d_fields || !d_mean)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  if (n_members < 1 || count == 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or count = 0");
  if (ld_fine < count)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": ld_fine shorter than a field of count entries");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  hipLaunchKernelGGL(k_ens_moments, lod_flat_grid(count), dim3(256), 0, st, d_fields, ld_fine, n_members, count, d_mean, d_var);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

} // extern "C"
#pragma GCC visibility pop
