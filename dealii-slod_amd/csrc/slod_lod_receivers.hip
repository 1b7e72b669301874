// Observation on the LOD space (the reference has no counterpart: it writes the whole fine field, LOD.cc:1005-1040):
//   slod_lod_receivers_create   rows of  O = W C  over the coarse unknowns for a few weighted fine dofs, CSR, from the slab
//   slod_lod_observe_multi      y = O u  on a coarse multi-vector, one row set for every column
//   slod_lod_observe_ensemble   the same with the values of member m for column m
//   slod_lod_time_record_arm    the product recorded inside the next time loop (slod_lod_time/wave/irk.hip)
// A term (fine node, component c, weight w) contributes, in the order of lod_reconstruct_node (slod_lod_system.hip.h: the
// centre cells cy, then cx, of the patches that hold the node, then d), the column p s + d with the value w phi_{p,d}(node, c).
// The host walks that loop once per term for the columns and the slab offsets (slod_grid.hip.h); k_receiver_rows gathers the
// values, member-minor; k_lod_observe runs one fma chain per (receiver, column) over the row in its order, so a one-term
// receiver of weight 1 has the 64-bit word slod_lod_reconstruct_multi / _ensemble writes at that node and component.
#include "slod_grid.hip.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace
{
  constexpr int OBS_AHEAD = 8; // entries whose loads are issued before the first fma

  // values[e K + m] = w_e basis[m member_stride + off_e]: one rounding
  __global__ __launch_bounds__(256) void k_receiver_rows(size_t nnz, int K, const double *__restrict__ weight,
                                                        const uint64_t *__restrict__ off, const double *__restrict__ basis,
                                                        size_t member_stride, double *__restrict__ values)
  {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nnz * (size_t)K)
      return;
    const size_t e = t / (size_t)K, m = t - e * (size_t)K;
    values[t]      = weight[e] * basis[m * member_stride + off[e]];
  }

  // One thread per (receiver q, column c), columns on adjacent lanes; blockIdx.y = the quantity (0: x0, 1: x1), written at
  // y[((blockIdx.y n_recv) + q) ld_y + c].  PER_COL: column c reads the values of member m0 + c, else every column member m0.
  // The chain acc = fma(value_e, x[cols_e ld + c], acc) runs from 0.0 over the row in order; the loads of OBS_AHEAD entries
  // are issued before the first fma, an entry past the end of the row reads the last one and adds nothing.
  template <bool PER_COL>
  __global__ __launch_bounds__(256) void k_lod_observe(int n_recv, int n, int K, int m0, const uint32_t *__restrict__ row_begin,
                                                      const uint32_t *__restrict__ cols, const double *__restrict__ values,
                                                      const double *__restrict__ x0, size_t ld0, const double *__restrict__ x1,
                                                      size_t ld1, double *__restrict__ y, size_t ld_y)
  {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n_recv * n)
      return;
    const int     q = (int)(t / n), c = (int)(t - (size_t)q * n);
    const double *x = blockIdx.y ? x1 : x0;
    const size_t  ld = blockIdx.y ? ld1 : ld0;
    const size_t  mv = (size_t)m0 + (PER_COL ? (size_t)c : 0);
    const uint32_t b = row_begin[q], end = row_begin[q + 1];
    double         acc = 0.0;
    for (uint32_t e0 = b; e0 < end; e0 += OBS_AHEAD)
      {
        double val[OBS_AHEAD], xv[OBS_AHEAD];
#pragma unroll
        for (int u = 0; u < OBS_AHEAD; ++u)
          {
            const uint32_t e = min(e0 + u, end - 1);
            val[u]           = values[(size_t)e * K + mv];
            xv[u]            = x[(size_t)cols[e] * ld + c];
          }
#pragma unroll
        for (int u = 0; u < OBS_AHEAD; ++u)
          {
            const double tt = fma(val[u], xv[u], acc);
            acc             = e0 + u < end ? tt : acc;
          }
      }
    y[((size_t)blockIdx.y * n_recv + q) * ld_y + c] = acc;
  }

  // The row of one term in row order: columns, and (offs given) the offsets of its words in a slab of the given stride
  int term_row(const SlodGrid &G, uint32_t node, int comp, size_t stride, uint32_t *cols, uint64_t *offs, size_t capacity)
  {
    const int s = G.spacedim, n = G.n_sub, NEp = G.N * n + 1, l = G.oversampling;
    const int X = (int)(node % (uint32_t)NEp), Y = (int)(node / (uint32_t)NEp);
    const int cxl = std::max((X + n - 1) / n - 1 - l, 0), cxh = std::min(X / n + l, G.N - 1);
    const int cyl = std::max((Y + n - 1) / n - 1 - l, 0), cyh = std::min(Y / n + l, G.N - 1);
    size_t    cnt = 0;
    for (int cy = cyl; cy <= cyh; ++cy)
      for (int cx = cxl; cx <= cxh; ++cx)
        {
          const Extent e = grid_extent(G, cx, cy);
          const int    ix = X - e.x0 * n, iy = Y - e.y0 * n;
          if (ix < 0 || ix > e.mx * n || iy < 0 || iy > e.my * n)
            continue;
          const uint32_t p   = grid_pid(G, cx, cy);
          const int      pnx = e.mx * n + 1, pnf = s * pnx * (e.my * n + 1);
          for (int d = 0; d < s; ++d, ++cnt)
            {
              if (cnt >= capacity)
                return -1;
              cols[cnt] = p * (uint32_t)s + (uint32_t)d;
              if (offs)
                offs[cnt] = (uint64_t)p * stride + (uint64_t)d * pnf + (uint64_t)s * (ix + iy * pnx) + (uint64_t)comp;
            }
        }
    return (int)cnt;
  }

  int receiver_capacity(const SlodGrid &G) { return (2 * G.oversampling + 2) * (2 * G.oversampling + 2) * G.spacedim; }

  // the words of the largest patch of the handle: s vectors on (m n + 1)^2 nodes of s components, m = min(2 l + 1, N)
  size_t patch_words(const slod_handle *h)
  {
    const size_t s = (size_t)h->cfg.spacedim, m = (size_t)std::min(2 * h->cfg.oversampling + 1, h->N);
    const size_t side = m * (size_t)h->cfg.n_subdivisions + 1;
    return s * s * side * side;
  }

  void observe_launch(hipStream_t st, const slod_lod_receivers *r, bool per_col, int m0, int n, int nq, const double *x0, size_t ld0,
                      const double *x1, size_t ld1, double *y, size_t ld_y)
  {
    const dim3 grid((unsigned)(((size_t)r->n_recv * n + 255) / 256), (unsigned)nq);
    hipLaunchKernelGGL(per_col ? k_lod_observe<true> : k_lod_observe<false>, grid, dim3(256), 0, st, r->n_recv, n, r->n_members, m0,
                       r->row_begin, r->cols, r->values, x0, ld0, x1, ld1, y, ld_y);
  }

  // the body of the two observe calls
  int observe(slod_handle *h, const std::string &who, const slod_lod_receivers *r, bool per_col, int first_member, int n,
              const double *d_u, size_t ld_u, double *d_y, size_t ld_y, void *hip_stream)
  {
    if (!h)
      return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL handle");
    if (!r || !d_u || !d_y)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL receivers or array");
    if (n < 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (per_col ? ": n_members < 1" : ": n_rhs < 1"));
    if (const int rc = slod_check_ld(h, who.c_str(), per_col ? "n_members" : "n_rhs", n, {ld_u, ld_y}))
      return rc;
    if (r->h != h)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": receivers of another handle");
    if (!per_col && r->n_members != 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": receivers of another member count (takes an object of one member)");
    if (per_col && (first_member < 0 || first_member > r->n_members - n))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": members outside the receivers");
    hipStream_t st;
    if (const int rc = slod_enter(h, hip_stream, &st))
      return rc;
    observe_launch(st, r, per_col, per_col ? first_member : 0, n, 1, d_u, ld_u, d_u, ld_u, d_y, ld_y);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who.c_str());
  }
} // namespace

// ---- the record of a time loop (slod_host.h) ----
SlodLodRecord slod_lod_record_take(slod_handle *h)
{
  SlodLodRecord r;
  if (h && h->record_armed)
    {
      r.armed         = true;
      r.rec           = h->record;
      h->record_armed = false;
    }
  return r;
}

int slod_lod_record_check(const slod_handle *h, const std::string &who, SlodLodRecord *r, bool has_v, int n_steps, int n, bool per_col)
{
  if (!r->armed)
    return SLOD_OK;
  const slod_lod_time_record &t = r->rec;
  if ((t.what & SLOD_RECORD_V) && !has_v)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: SLOD_RECORD_V in a loop without a velocity");
  if (t.what < 1 || t.what > 3)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: what is SLOD_RECORD_U, SLOD_RECORD_V or both");
  if (t.every < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: every < 1");
  if (!t.d_trace)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: NULL d_trace");
  if (t.ld_trace < (size_t)n)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: ld_trace below " + (per_col ? "n_members" : "n_rhs"));
  r->nq = t.what == 3 ? 2 : 1;
  // record_stride < nq n_recv ld_trace, by division: the product of the three may not fit a size_t
  if (t.record_stride / ((size_t)r->nq * (size_t)t.recv->n_recv) < t.ld_trace)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: record_stride below n_quantities n_recv ld_trace");
  if (t.capacity < n_steps / t.every + 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: capacity below n_steps / every + 1");
  if (t.recv->h != h)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: receivers of another handle");
  if (t.recv->n_members != (per_col ? n : 1))
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": record: receivers of another member count");
  return SLOD_OK;
}

void slod_lod_record_launch(hipStream_t st, const SlodLodRecord &r, int j, int n, bool per_col, const double *d_u, size_t ld_u,
                            const double *d_v, size_t ld_v)
{
  const slod_lod_time_record &t = r.rec;
  const bool                  only_v = t.what == SLOD_RECORD_V;
  observe_launch(st, t.recv, per_col, 0, n, r.nq, only_v ? d_v : d_u, only_v ? ld_v : ld_u, d_v, ld_v,
                 t.d_trace + (size_t)j * t.record_stride, t.ld_trace);
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_receiver_capacity(const slod_handle *h)
{
  if (!h)
    return SLOD_ERR_ARGUMENT;
  return receiver_capacity(slod_grid_of(h));
}

int slod_lod_receiver_pattern(const slod_handle *h, uint32_t node, uint32_t *cols, size_t capacity)
{
  if (!h || !cols)
    return SLOD_ERR_ARGUMENT;
  if (node >= (uint32_t)(h->NE + 1) * (uint32_t)(h->NE + 1))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_receiver_pattern: node out of range");
  const int cnt = term_row(slod_grid_of(h), node, 0, 0, cols, nullptr, capacity);
  if (cnt < 0)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_receiver_pattern: buffer too small");
  return cnt;
}

int slod_lod_receivers_create(slod_handle *h, int n_recv, const uint32_t *term_begin, const uint32_t *term_node,
                              const int32_t *term_comp, const double *term_weight, const double *d_basis, size_t stride,
                              size_t member_stride, int n_members, slod_lod_receivers **out)
{
  const std::string who = "slod_lod_receivers_create";
  if (!h)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, who + ": NULL handle");
  if (!term_begin || !term_node || !term_comp || !term_weight || !d_basis || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL array or out");
  *out = nullptr;
  if (n_recv < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_recv < 1");
  if (n_members < 1 || n_members > 65535)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_members < 1 or > 65535");
  if (stride < patch_words(h))
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": stride below the words of a patch");
  for (int q = 0; q < n_recv; ++q)
    {
      if (term_begin[q + 1] < term_begin[q] || (q == 0 && term_begin[0] != 0))
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": term_begin does not start at 0 or is not monotone");
      if (term_begin[q + 1] == term_begin[q])
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": receiver " + std::to_string(q) + " has no term");
    }
  const SlodGrid G = slod_grid_of(h);
  const uint32_t n_node = (uint32_t)(h->NE + 1) * (uint32_t)(h->NE + 1), n_term = term_begin[n_recv];
  const int      cap = receiver_capacity(G);
  std::vector<uint32_t> tc((size_t)cap);
  std::vector<uint64_t> to((size_t)cap);
  uint64_t              total = 0, last_count = 0;
  for (uint32_t t = 0; t < n_term; ++t)
    {
      if (term_node[t] >= n_node)
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": term " + std::to_string(t) + ": node out of range");
      if (term_comp[t] < 0 || term_comp[t] >= G.spacedim)
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": term " + std::to_string(t) + ": component out of range");
      if (!std::isfinite(term_weight[t]))
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": term " + std::to_string(t) + ": weight is not finite");
      if (t == 0 || term_node[t] != term_node[t - 1]) // the count depends on the node alone
        last_count = (uint64_t)term_row(G, term_node[t], 0, 0, tc.data(), nullptr, (size_t)cap);
      total += last_count;
      if (total > 0x7fffffffull)
        return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": nnz does not fit 31 bits");
    }
  // rows, from the grid alone
  std::vector<uint32_t> row_begin((size_t)n_recv + 1, 0), cols;
  std::vector<uint64_t> offs;
  std::vector<double>   weight;
  cols.reserve((size_t)total), offs.reserve((size_t)total), weight.reserve((size_t)total);
  for (int q = 0; q < n_recv; ++q)
    {
      for (uint32_t t = term_begin[q]; t < term_begin[q + 1]; ++t)
        {
          const int cnt = term_row(G, term_node[t], term_comp[t], stride, tc.data(), to.data(), (size_t)cap);
          cols.insert(cols.end(), tc.begin(), tc.begin() + cnt);
          offs.insert(offs.end(), to.begin(), to.begin() + cnt);
          weight.insert(weight.end(), (size_t)cnt, term_weight[t]);
        }
      row_begin[(size_t)q + 1] = (uint32_t)cols.size();
    }
  const size_t nnz = cols.size();
  hipStream_t  st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  slod_lod_receivers *r = new slod_lod_receivers;
  r->h = h, r->n_recv = n_recv, r->n_members = n_members, r->nnz = nnz;
  // values first (doubles), then the two index arrays
  const size_t nval = nnz * (size_t)n_members;
  r->bytes          = nval * sizeof(double) + (nnz + (size_t)n_recv + 1) * sizeof(uint32_t);
  SlodDevBuf<char> tmp; // weights and offsets of the gather
  hipError_t       e = r->mem.alloc(r->bytes);
  if (e == hipSuccess)
    e = tmp.alloc(nnz * (sizeof(double) + sizeof(uint64_t)));
  if (e == hipSuccess)
    {
      r->values    = (double *)r->mem.get();
      r->cols      = (uint32_t *)(r->values + nval);
      r->row_begin = r->cols + nnz;
      double   *d_w = (double *)tmp.get();
      uint64_t *d_o = (uint64_t *)(d_w + nnz);
      e             = hipMemcpyAsync(r->cols, cols.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(r->row_begin, row_begin.data(), row_begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(d_w, weight.data(), nnz * sizeof(double), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(d_o, offs.data(), nnz * sizeof(uint64_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        {
          hipLaunchKernelGGL(k_receiver_rows, dim3((unsigned)((nval + 255) / 256)), dim3(256), 0, st, nnz, n_members, d_w, d_o, d_basis,
                             member_stride, r->values);
          e = hipGetLastError();
        }
      const hipError_t es = hipStreamSynchronize(st); // the host vectors and tmp go on return
      if (e == hipSuccess)
        e = es;
    }
  if (e != hipSuccess)
    {
      delete r;
      return slod_hip_fail(h, e, who.c_str());
    }
  *out = r;
  return SLOD_OK;
}

int slod_lod_receivers_get_info(const slod_lod_receivers *r, slod_lod_receivers_info *info)
{
  if (!r || !info)
    return SLOD_ERR_ARGUMENT;
  info->n_receivers = r->n_recv;
  info->n_members   = r->n_members;
  info->nnz         = (uint64_t)r->nnz;
  info->bytes       = (uint64_t)r->bytes;
  return SLOD_OK;
}

int slod_lod_receivers_rows(const slod_lod_receivers *r, int member, uint32_t *row_begin, uint32_t *cols, double *values)
{
  if (!r)
    return SLOD_ERR_ARGUMENT;
  slod_handle      *h = r->h;
  const std::string who = "slod_lod_receivers_rows";
  if (!row_begin || !cols || !values)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": NULL array");
  if (member < 0 || member >= r->n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": member outside the receivers");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  hipError_t e = hipStreamSynchronize(st);
  if (e == hipSuccess)
    e = hipMemcpy(row_begin, r->row_begin, ((size_t)r->n_recv + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy(cols, r->cols, r->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy2D(values, sizeof(double), r->values + member, (size_t)r->n_members * sizeof(double), sizeof(double), r->nnz,
                    hipMemcpyDeviceToHost);
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who.c_str());
}

void slod_lod_receivers_destroy(slod_lod_receivers *r)
{
  if (!r)
    return;
  if (r->h->record_armed && r->h->record.recv == r)
    r->h->record_armed = false; // a record armed on these receivers goes with them
  (void)hipSetDevice(r->h->cfg.device);
  (void)hipDeviceSynchronize(); // a product on the handle's stream or on a caller's may still read the rows
  delete r;
}

int slod_lod_observe_multi(slod_handle *h, const slod_lod_receivers *recv, const double *d_u, size_t ld_u, int n_rhs, double *d_y,
                           size_t ld_y, void *hip_stream)
{
  return observe(h, "slod_lod_observe_multi", recv, false, 0, n_rhs, d_u, ld_u, d_y, ld_y, hip_stream);
}

int slod_lod_observe_ensemble(slod_handle *h, const slod_lod_receivers *recv, int first_member, int n_members, const double *d_u,
                              size_t ld_u, double *d_y, size_t ld_y, void *hip_stream)
{
  return observe(h, "slod_lod_observe_ensemble", recv, true, first_member, n_members, d_u, ld_u, d_y, ld_y, hip_stream);
}

int slod_lod_time_record_arm(slod_handle *h, const slod_lod_time_record *rec)
{
  if (!h)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, "slod_lod_time_record_arm: NULL handle");
  if (!rec)
    {
      h->record_armed = false;
      return SLOD_OK;
    }
  if (!rec->recv)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_time_record_arm: NULL recv");
  h->record       = *rec;
  h->record_armed = true;
  return SLOD_OK;
}

} // extern "C"
#pragma GCC visibility pop
