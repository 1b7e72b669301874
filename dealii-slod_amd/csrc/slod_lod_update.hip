// Refresh after a local coefficient change (the reference has no counterpart: its coefficient is fixed for the life
// of a basis, LOD.cc:296-768).  A patch basis depends on the coefficient inside its own patch only, so a change in a
// small part of the domain leaves most patches, and most entries of A_LOD and M_LOD, as they are:
//   slod_update_coefficient      stores the new field and flags the patches whose extent holds a changed fine element
//   slod_dirty_patches           the flagged patches on the host
//   slod_plan_create_dirty       the plan that overwrites the flagged patches of a uniform-stride slab in place
//   slod_lod_matrix_update       the entries of A_LOD with a flagged row or column, in place
//   slod_lod_mass_matrix_update  the same for M_LOD
// The two matrix kernels run the per-slot bodies of the full-row kernels (slod_lod_system.hip.h): an entry is the
// work of one wave in a fixed order, so a recomputed entry has the bits of a full rebuild on the same slabs.
#include "slod_lod_system.hip.h"

#include <vector>

namespace
{
  // ---------------------------------------------------------------------------------
  // Compare and store.  Block = one coarse cell, threads over its n x n fine elements x 4 stored values.  LAYOUT 1:
  // data[NE][NE][4]; LAYOUT 0: data[NE][NE], the value of an element against each of its four slots.  The comparison
  // is on the 64-bit words: any other bit pattern is a change (also -0 against +0, and one NaN against another).
  // cell_flag[cx + N cy] = 1 when a value of the cell changed, else 0 (every block writes its word).
  // ---------------------------------------------------------------------------------
  template <int LAYOUT>
  __global__ __launch_bounds__(256) void k_coef_update(int N, int n, const double *data, double *stored, uint32_t *cell_flag)
  {
    const int cx = blockIdx.x % N, cy = blockIdx.x / N, NE = N * n;
    int       changed = 0;
    for (int t = threadIdx.x; t < n * n * 4; t += 256)
      {
        const int    q = t & 3, el = t >> 2, iy = el / n, ix = el - iy * n;
        const size_t elem = (size_t)(cy * n + iy) * NE + (cx * n + ix);
        const double v = LAYOUT == 1 ? data[elem * 4 + q] : data[elem];
        if (__double_as_longlong(v) != __double_as_longlong(stored[elem * 4 + q]))
          {
            stored[elem * 4 + q] = v;
            changed              = 1;
          }
      }
    changed = __syncthreads_or(changed);
    if (threadIdx.x == 0)
      cell_flag[blockIdx.x] = changed ? 1u : 0u;
  }

  // One thread per patch: OR of the flags of the cells of its extent into its word (clean patches are not written)
  __global__ __launch_bounds__(256) void k_mark_dirty(const SlodGrid G, int NP, const uint32_t *cell_flag, uint32_t *dirty)
  {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= NP)
      return;
    int cx, cy;
    grid_centre(G, (uint32_t)p, cx, cy);
    const Extent e = grid_extent(G, cx, cy);
    uint32_t     any = 0;
    for (int y = e.y0; y < e.y0 + e.my; ++y)
      for (int x = e.x0; x < e.x0 + e.mx; ++x)
        any |= cell_flag[x + G.N * y];
    if (any)
      dirty[p] |= 1u;
  }

  // ---------------------------------------------------------------------------------
  // In-place update of a full set of block rows.  Block = row patch p, wave w = the slots j = w, w+4, ... as in
  // k_lod_matrix.  A used slot (p, j) with column q is recomputed when p or q is flagged; every other word of the
  // values is left alone.  A clean row far from any flagged patch costs its cap flag loads.
  // ---------------------------------------------------------------------------------
  __global__ __launch_bounds__(256) void k_lod_matrix_update(const SlodGrid G, const uint32_t *dirty, const double *basis,
                                                            const double *premult, size_t stride, double *values, size_t ld)
  {
    const int      wave = threadIdx.x >> 6, cap = grid_row_capacity(G);
    const uint32_t p = blockIdx.x;
    int            pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent   pe = grid_extent(G, pcx, pcy);
    const double  *phi = basis + (size_t)p * stride;
    const uint32_t row_dirty = dirty[p];
    for (int j = wave; j < cap; j += 4)
      {
        const PairGeom pg = grid_pair(G, pcx, pcy, pe, j);
        const uint32_t q  = pg.col();
        if (q == 0xffffffffu || !(row_dirty | dirty[q]))
          continue; // wave-uniform
        lod_matrix_slot(G, pe, phi, pg, premult, stride, (size_t)p * cap + j, values, ld);
      }
  }

  template <int S>
  __global__ __launch_bounds__(256) void k_lod_mass_update(const SlodGrid G, const uint32_t *dirty, const double *basis,
                                                          size_t stride, const double *rho, double scale, double *values)
  {
    const int      wave = threadIdx.x >> 6, cap = grid_row_capacity(G);
    const uint32_t p = blockIdx.x;
    int            pcx, pcy;
    grid_centre(G, p, pcx, pcy);
    const Extent   pe = grid_extent(G, pcx, pcy);
    const double  *phi = basis + (size_t)p * stride;
    const uint32_t row_dirty = dirty[p];
    for (int j = wave; j < cap; j += 4)
      {
        const PairGeom pg = grid_pair(G, pcx, pcy, pe, j);
        const uint32_t q  = pg.col();
        if (q == 0xffffffffu || !(row_dirty | dirty[q]))
          continue; // wave-uniform
        lod_mass_slot<S>(G, pe, phi, pg, basis, stride, rho, scale, (size_t)p * cap + j, values, 1);
      }
  }

  // the flags of all patches on the host, after everything the handle's stream holds; the handle's device is current
  hipError_t read_dirty(slod_handle *h, const uint32_t *d_dirty, std::vector<uint32_t> *flags)
  {
    flags->assign((size_t)h->NP, 0u);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess)
      e = hipMemcpy(flags->data(), d_dirty, flags->size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return e;
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_update_coefficient(slod_handle *h, uint32_t problem, int field, const double *data, int layout, size_t count,
                            int on_device, uint32_t *d_dirty)
{
  const char *who = "slod_update_coefficient";
  if (!h || !data || !d_dirty)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  if (problem >= (uint32_t)h->cfg.n_problems || field < 0 || field >= h->cfg.spacedim)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": problem/field out of range");
  const size_t ne = (size_t)h->NE * h->NE;
  if ((layout == 0 && count != ne) || (layout == 1 && count != 4 * ne) || (layout != 0 && layout != 1))
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": wrong element count for layout");
  if (h->cfg.constant_coefficients)
    return slod_fail(h, SLOD_ERR_UNSUPPORTED,
                     std::string(who) + ": with constant_coefficients every full patch reads the first full patch's tile");
  if (!h->coef_set[(size_t)problem * 2 + field])
    return slod_fail(h, SLOD_ERR_STATE, std::string(who) + ": coefficient field not set (slod_set_coefficient comes first)");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  // the staging copy of host data and the flags of the coarse cells are owned by the call
  SlodDevBuf<double>   staging;
  SlodDevBuf<uint32_t> cell_flag;
  hipError_t           e = cell_flag.alloc((size_t)h->NP);
  if (e == hipSuccess && !on_device)
    {
      e = staging.alloc(count);
      if (e == hipSuccess)
        e = hipMemcpyAsync(staging.get(), data, count * sizeof(double), hipMemcpyHostToDevice, st);
      data = staging.get();
    }
  if (e == hipSuccess)
    {
      double *stored = h->d_coef[field] + (size_t)problem * ne * 4;
      if (layout == 1)
        hipLaunchKernelGGL(k_coef_update<1>, dim3((unsigned)h->NP), dim3(256), 0, st, h->N, h->cfg.n_subdivisions, data, stored,
                           cell_flag.get());
      else
        hipLaunchKernelGGL(k_coef_update<0>, dim3((unsigned)h->NP), dim3(256), 0, st, h->N, h->cfg.n_subdivisions, data, stored,
                           cell_flag.get());
      hipLaunchKernelGGL(k_mark_dirty, dim3((unsigned)((h->NP + 255) / 256)), dim3(256), 0, st, slod_grid_of(h), h->NP,
                         cell_flag.get(), d_dirty);
      e = hipGetLastError();
    }
  // (also when a launch failed: the buffers of the call are freed on return)
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess)
    e = es;
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_dirty_patches(slod_handle *h, const uint32_t *d_dirty, uint32_t *patches, size_t capacity)
{
  const char *who = "slod_dirty_patches";
  if (!h || !d_dirty)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  if (const int rc = slod_enter(h, nullptr, nullptr))
    return rc;
  std::vector<uint32_t> flags;
  if (const hipError_t e = read_dirty(h, d_dirty, &flags); e != hipSuccess)
    return slod_hip_fail(h, e, who);
  size_t count = 0;
  for (const uint32_t f : flags)
    count += f != 0;
  if (patches)
    {
      if (capacity < count)
        return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": buffer too small");
      size_t k = 0;
      for (size_t p = 0; p < flags.size(); ++p)
        if (flags[p])
          patches[k++] = (uint32_t)p;
    }
  return (int)count;
}

int slod_plan_create_dirty(slod_handle *h, uint32_t problem, const uint32_t *d_dirty, slod_plan **out)
{
  const char *who = "slod_plan_create_dirty";
  if (!h || !d_dirty || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle, array or output");
  *out = nullptr;
  if (problem >= (uint32_t)h->cfg.n_problems)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": problem out of range");
  if (const int rc = slod_enter(h, nullptr, nullptr))
    return rc;
  std::vector<uint32_t> flags;
  if (const hipError_t e = read_dirty(h, d_dirty, &flags); e != hipSuccess)
    return slod_hip_fail(h, e, who);
  std::vector<uint32_t> gids;
  std::vector<uint64_t> offsets;
  const size_t          stride = slod_uniform_stride(h);
  for (size_t p = 0; p < flags.size(); ++p)
    if (flags[p])
      {
        gids.push_back(problem * (uint32_t)h->NP + (uint32_t)p);
        offsets.push_back((uint64_t)p * stride);
      }
  if (const int rc = slod_plan_create(h, gids.data(), gids.size(), offsets.data(), out))
    return rc;
  return (int)gids.size();
}

int slod_lod_matrix_update(slod_handle *h, const uint32_t *d_dirty, const double *d_basis, const double *d_premult, size_t stride,
                           double *d_values, size_t ld_m, void *hip_stream)
{
  const char *who = "slod_lod_matrix_update";
  if (!h || !d_dirty || !d_basis || !d_premult || !d_values)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  if (ld_m < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": ld_m < 1");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  hipLaunchKernelGGL(k_lod_matrix_update, dim3((unsigned)h->NP), dim3(256), 0, st, slod_grid_of(h), d_dirty, d_basis, d_premult,
                     stride, d_values, ld_m);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_mass_matrix_update(slod_handle *h, const uint32_t *d_dirty, const double *d_basis, size_t stride, const double *d_rho,
                                double *d_values, void *hip_stream)
{
  const char *who = "slod_lod_mass_matrix_update";
  if (!h || !d_dirty || !d_basis || !d_values)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle or array");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const double hf = 1.0 / h->NE, scale = hf * hf / 36.0;
  if (h->cfg.spacedim == 1)
    hipLaunchKernelGGL(k_lod_mass_update<1>, dim3((unsigned)h->NP), dim3(256), 0, st, slod_grid_of(h), d_dirty, d_basis, stride,
                       d_rho, scale, d_values);
  else
    hipLaunchKernelGGL(k_lod_mass_update<2>, dim3((unsigned)h->NP), dim3(256), 0, st, slod_grid_of(h), d_dirty, d_basis, stride,
                       d_rho, scale, d_values);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

} // extern "C"
#pragma GCC visibility pop
