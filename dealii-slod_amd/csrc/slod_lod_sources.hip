// Point sources on the LOD space (the reference has no counterpart: its one load is assembled on the fine mesh):
//   slod_lod_sources_create    the rows of a receivers object transposed: per touched coarse row its entries, by source
//   slod_lod_inject_multi      b = base + O^T g  on a coarse multi-vector, one value set for every column
//   slod_lod_inject_ensemble   the same with the values of member m for column m
//   slod_lod_time_source_arm   the product as the load of the next time loop (slod_lod_time/wave/irk.hip)
// A point force w e(node, c) has the coarse load C^T w e, the row of O = W C that slod_lod_receivers_create gathers, so
// source q is receiver q and the object is the CSR of the receivers regrouped by column on the host: the touched coarse
// rows ascending, per row the entries e with cols[e] = r in ascending e.  k_source_cols copies the values into that order,
// member-minor; k_lod_inject runs one fma chain per (coarse row, column) from the base word over the row's entries, so a
// one-term source of weight 1 and signal 1 leaves the words slod_lod_rhs_multi has for the fine field e(node, c).
#include "slod_host.h"

#include <string>
#include <vector>

namespace
{
  constexpr int INJ_AHEAD = 8; // entries whose loads are issued before the first fma

  // values[i K + m] = from[perm[i] K + m]: a copy
  __global__ __launch_bounds__(256) void k_source_cols(size_t nnz, int K, const uint32_t *__restrict__ perm,
                                                      const double *__restrict__ from, double *__restrict__ values)
  {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nnz * (size_t)K)
      return;
    const size_t i = t / (size_t)K, m = t - i * (size_t)K;
    values[t]      = from[(size_t)perm[i] * K + m];
  }

  // One thread per (coarse row r, column c), columns on adjacent lanes; blockIdx.y = the sample of the launch: g, base and b
  // advance by their sample strides.  An untouched row (slot < 0) writes its base word, +0.0 without a base.  A touched row
  // runs acc = fma(value_i, g[src_i ld_g + c], acc) from the base word over its entries in order; the loads of INJ_AHEAD
  // entries are issued before the first fma, an entry past the end of the row reads the last one and adds nothing.
  // PER_COL: column c reads the values of member m0 + c, else every column member m0.  b may be base: a thread reads its
  // own word before it writes it (no __restrict__ on the two).
  template <bool PER_COL>
  __global__ __launch_bounds__(256) void k_lod_inject(int nrow, int n, int K, int m0, const int32_t *__restrict__ slot,
                                                     const uint32_t *__restrict__ begin, const uint32_t *__restrict__ src,
                                                     const double *__restrict__ values, const double *__restrict__ g, size_t ld_g,
                                                     size_t g_stride, const double *base, size_t ld_base, size_t base_stride,
                                                     double *b, size_t ld_b, size_t b_stride)
  {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nrow * n)
      return;
    const int    r = (int)(t / n), c = (int)(t - (size_t)r * n);
    const size_t y = blockIdx.y;
    double       acc = base ? base[y * base_stride + (size_t)r * ld_base + c] : 0.0;
    const int32_t sl = slot[r];
    if (sl >= 0)
      {
        const double  *gy = g + y * g_stride;
        const size_t   mv = (size_t)m0 + (PER_COL ? (size_t)c : 0);
        const uint32_t b0 = begin[sl], end = begin[sl + 1];
        for (uint32_t i0 = b0; i0 < end; i0 += INJ_AHEAD)
          {
            double val[INJ_AHEAD], gv[INJ_AHEAD];
#pragma unroll
            for (int u = 0; u < INJ_AHEAD; ++u)
              {
                const uint32_t i = min(i0 + u, end - 1);
                val[u]           = values[(size_t)i * K + mv];
                gv[u]            = gy[(size_t)src[i] * ld_g + c];
              }
#pragma unroll
            for (int u = 0; u < INJ_AHEAD; ++u)
              {
                const double tt = fma(val[u], gv[u], acc);
                acc             = i0 + u < end ? tt : acc;
              }
          }
      }
    b[y * b_stride + (size_t)r * ld_b + c] = acc;
  }

  void inject_launch(hipStream_t st, const slod_lod_sources *s, bool per_col, int m0, int n, int ny, const double *g, size_t ld_g,
                     size_t g_stride, const double *base, size_t ld_base, size_t base_stride, double *b, size_t ld_b, size_t b_stride)
  {
    const dim3 grid((unsigned)(((size_t)s->nrow * n + 255) / 256), (unsigned)ny);
    hipLaunchKernelGGL(per_col ? k_lod_inject<true> : k_lod_inject<false>, grid, dim3(256), 0, st, s->nrow, n, s->n_members, m0,
                       s->slot, s->begin, s->src, s->values, g, ld_g, g_stride, base, ld_base, base_stride, b, ld_b, b_stride);
  }

  // the body of the two inject calls
  int inject(slod_handle *h, const std::string &who, const slod_lod_sources *s, bool per_col, int first_member, int n,
             const double *d_g, size_t ld_g, const double *d_base, size_t ld_base, double *d_b, size_t ld_b, void *hip_stream)
  {
    if (!h)
      return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL handle");
    if (!s || !d_g || !d_b)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL sources or array");
    if (n < 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (per_col ? ": n_members < 1" : ": n_rhs < 1"));
    if (const int rc = slod_check_ld(h, who.c_str(), per_col ? "n_members" : "n_rhs", n, {ld_g, ld_b, d_base ? ld_base : ld_b}))
      return rc;
    if (s->h != h)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": sources of another handle");
    if (!per_col && s->n_members != 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": sources of another member count (takes an object of one member)");
    if (per_col && (first_member < 0 || first_member > s->n_members - n))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": members outside the sources");
    hipStream_t st;
    if (const int rc = slod_enter(h, hip_stream, &st))
      return rc;
    inject_launch(st, s, per_col, per_col ? first_member : 0, n, 1, d_g, ld_g, 0, d_base, ld_base, 0, d_b, ld_b, 0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who.c_str());
  }
} // namespace

// ---- the source of a time loop (slod_host.h) ----
SlodLodSource slod_lod_source_take(slod_handle *h)
{
  SlodLodSource s;
  if (h && h->source_armed)
    {
      s.armed         = true;
      s.s             = h->source;
      h->source_armed = false;
    }
  return s;
}

int slod_lod_source_check(const slod_handle *h, const std::string &who, const SlodLodSource &s, int need, const char *bound, int n,
                          bool per_col)
{
  if (!s.armed)
    return SLOD_OK;
  const slod_lod_time_source &t = s.s;
  if (!t.d_signal)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": source: NULL d_signal");
  if (t.ld_signal < (size_t)n)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": source: ld_signal below " + (per_col ? "n_members" : "n_rhs"));
  // sample_stride < n_sources ld_signal, by division: the product may not fit a size_t
  if (t.sample_stride / (size_t)t.src->n_src < t.ld_signal)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": source: sample_stride below n_sources ld_signal");
  if (t.n_samples < need)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": source: n_samples below " + bound);
  if (t.src->h != h)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": source: sources of another handle");
  if (t.src->n_members != (per_col ? n : 1))
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": source: sources of another member count");
  return SLOD_OK;
}

void slod_lod_source_launch(hipStream_t st, const SlodLodSource &s, int sample, int ny, int n, bool per_col, const double *d_base,
                            size_t ld_base, size_t base_stride, double *d_b, size_t b_stride)
{
  const slod_lod_time_source &t = s.s;
  inject_launch(st, t.src, per_col, 0, n, ny, t.d_signal + (size_t)sample * t.sample_stride, t.ld_signal, t.sample_stride, d_base,
                ld_base, base_stride, d_b, (size_t)n, b_stride);
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_sources_create(slod_handle *h, const slod_lod_receivers *recv, slod_lod_sources **out)
{
  const std::string who = "slod_lod_sources_create";
  if (!h)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL handle");
  if (!recv || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL recv or out");
  *out = nullptr;
  if (recv->h != h)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": receivers of another handle");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const size_t          nnz = recv->nnz, K = (size_t)recv->n_members;
  const int             nrow = h->NP * h->cfg.spacedim;
  std::vector<uint32_t> row_begin((size_t)recv->n_recv + 1), cols(nnz);
  hipError_t            e = hipStreamSynchronize(st); // a receivers object is complete when its create returns; a caller's product may run
  if (e == hipSuccess)
    e = hipMemcpy(row_begin.data(), recv->row_begin, row_begin.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy(cols.data(), recv->cols, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who.c_str());
  // the transposed index: a counting sort of the entries by column keeps them in ascending e
  std::vector<int32_t>  slot((size_t)nrow, -1);
  std::vector<uint32_t> count((size_t)nrow, 0);
  for (size_t k = 0; k < nnz; ++k)
    ++count[cols[k]];
  std::vector<uint32_t> begin(1, 0);
  for (int r = 0; r < nrow; ++r)
    if (count[(size_t)r])
      {
        slot[(size_t)r] = (int32_t)begin.size() - 1;
        begin.push_back(begin.back() + count[(size_t)r]);
      }
  const uint32_t        n_touched = (uint32_t)begin.size() - 1;
  std::vector<uint32_t> fill(begin.begin(), begin.end() - 1), perm(nnz), src(nnz);
  for (int q = 0; q < recv->n_recv; ++q)
    for (uint32_t k = row_begin[(size_t)q]; k < row_begin[(size_t)q + 1]; ++k)
      {
        const uint32_t i = fill[(size_t)slot[cols[k]]]++;
        perm[i] = k, src[i] = (uint32_t)q;
      }
  slod_lod_sources *s = new slod_lod_sources;
  s->h = h, s->n_src = recv->n_recv, s->n_members = recv->n_members, s->nrow = nrow, s->n_touched = n_touched, s->nnz = nnz;
  // values first (doubles), then the index arrays
  const size_t nval = nnz * K;
  s->bytes          = nval * sizeof(double) + ((size_t)n_touched + 1 + nnz + (size_t)nrow) * sizeof(uint32_t);
  SlodDevBuf<uint32_t> d_perm;
  e = s->mem.alloc(s->bytes);
  if (e == hipSuccess)
    e = d_perm.alloc(std::max<size_t>(nnz, 1));
  if (e == hipSuccess)
    {
      s->values = (double *)s->mem.get();
      s->begin  = (uint32_t *)(s->values + nval);
      s->src    = s->begin + n_touched + 1;
      s->slot   = (int32_t *)(s->src + nnz);
      e         = hipMemcpyAsync(s->begin, begin.data(), begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(s->src, src.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(s->slot, slot.data(), (size_t)nrow * sizeof(int32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(d_perm.get(), perm.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess && nval)
        {
          hipLaunchKernelGGL(k_source_cols, dim3((unsigned)((nval + 255) / 256)), dim3(256), 0, st, nnz, (int)K, d_perm.get(),
                             recv->values, s->values);
          e = hipGetLastError();
        }
      const hipError_t es = hipStreamSynchronize(st); // the host vectors and d_perm go on return
      if (e == hipSuccess)
        e = es;
    }
  if (e != hipSuccess)
    {
      delete s;
      return slod_hip_fail(h, e, who.c_str());
    }
  *out = s;
  return SLOD_OK;
}

int slod_lod_sources_get_info(const slod_lod_sources *s, slod_lod_sources_info *info)
{
  if (!s || !info)
    return SLOD_ERR_ARGUMENT;
  info->n_sources      = s->n_src;
  info->n_members      = s->n_members;
  info->n_rows_touched = s->n_touched;
  info->nnz            = (uint64_t)s->nnz;
  info->bytes          = (uint64_t)s->bytes;
  return SLOD_OK;
}

void slod_lod_sources_destroy(slod_lod_sources *s)
{
  if (!s)
    return;
  if (s->h->source_armed && s->h->source.src == s)
    s->h->source_armed = false; // a source armed on this object goes with it
  (void)hipSetDevice(s->h->cfg.device);
  (void)hipDeviceSynchronize(); // a product on the handle's stream or on a caller's may still read the object
  delete s;
}

int slod_lod_inject_multi(slod_handle *h, const slod_lod_sources *src, const double *d_g, size_t ld_g, int n_rhs, const double *d_base,
                          size_t ld_base, double *d_b, size_t ld_b, void *hip_stream)
{
  return inject(h, "slod_lod_inject_multi", src, false, 0, n_rhs, d_g, ld_g, d_base, ld_base, d_b, ld_b, hip_stream);
}

int slod_lod_inject_ensemble(slod_handle *h, const slod_lod_sources *src, int first_member, int n_members, const double *d_g,
                             size_t ld_g, const double *d_base, size_t ld_base, double *d_b, size_t ld_b, void *hip_stream)
{
  return inject(h, "slod_lod_inject_ensemble", src, true, first_member, n_members, d_g, ld_g, d_base, ld_base, d_b, ld_b, hip_stream);
}

int slod_lod_time_source_arm(slod_handle *h, const slod_lod_time_source *s)
{
  if (!h)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, "slod_lod_time_source_arm: NULL handle");
  if (!s)
    {
      h->source_armed = false;
      return SLOD_OK;
    }
  if (!s->src)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_time_source_arm: NULL src");
  h->source       = *s;
  h->source_armed = true;
  return SLOD_OK;
}

} // extern "C"
#pragma GCC visibility pop
