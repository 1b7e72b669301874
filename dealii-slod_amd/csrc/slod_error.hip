// Error norms of e = u - v - w on the global fine grid (the reference's compare_lod_with_fem,
// LOD.cc:1240-1260, and error_FEMh_exact, LOD.cc:1080-1088): L2, H1-seminorm and max over the
// quadrature points per component, and the energy a(e,e) with the coefficient of the handle.
// Quadrature: the 2 x 2 Gauss rule on every fine element (QIterated(QGauss(2), n), LOD.cc:91-92),
// points q = q0 + 2 q1 in the order of slod_set_coefficient layout 1.
//
// One thread per fine element of a run of 256, ex fastest (corner loads of neighbouring lanes coalesce);
// on large grids a block walks several runs (at most 2048 partials up to NE = 5792).  HBM-bound:
// per element 4 coefficient values per field and, with an exact function, 4 (1 + 2) values per
// component, read as 16-byte loads.  The reduction is deterministic: wave shuffles, then the four
// waves of a block combined in LDS in a fixed order, one partial per block in block order; a second,
// single-block pass combines the partials in a fixed order.  No atomics.
#include "slod_host.h"

#include <algorithm>
#include <cmath>

namespace
{
  constexpr int ERR_BLOCK = 256;
  constexpr int ERR_SLOTS = 8; // per block: l2[2], h1[2], linf[2], energy, (unused)

  __device__ __forceinline__ bool slot_is_max(int k) { return k == 4 || k == 5; }

  __device__ __forceinline__ void load4(const double *p, double v[4])
  {
    const double2 a = *reinterpret_cast<const double2 *>(p);
    const double2 b = *reinterpret_cast<const double2 *>(p + 2);
    v[0]            = a.x;
    v[1]            = a.y;
    v[2]            = b.x;
    v[3]            = b.y;
  }

  __device__ __forceinline__ double wave_reduce(double v, bool is_max)
  {
    for (int off = 32; off > 0; off >>= 1)
      {
        const double o = __shfl_xor(v, off, 64);
        v              = is_max ? fmax(v, o) : v + o;
      }
    return v;
  }

  // r[k] of every lane -> block total of slot k (waves of NT threads in a fixed order); thread k < ERR_SLOTS holds it
  template <int NT>
  __device__ __forceinline__ double block_reduce(double r[ERR_SLOTS], double (*red)[ERR_SLOTS])
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < ERR_SLOTS; ++k)
      {
        const double t = wave_reduce(r[k], slot_is_max(k));
        if (lane == 0)
          red[wave][k] = t;
      }
    __syncthreads();
    double acc = 0.0;
    if (threadIdx.x < ERR_SLOTS)
      {
        const int k = threadIdx.x;
        acc         = red[0][k];
        for (int w = 1; w < NT / 64; ++w)
          acc = slot_is_max(k) ? fmax(acc, red[w][k]) : acc + red[w][k];
      }
    return acc;
  }

  // u, v: [(NE+1)^2][S] or null; wq: [S][NE][NE][4], wg: [S][2][NE][NE][4] (both or neither);
  // c0, c1: the coefficient fields of the problem, [NE][NE][4].  partial: [ERR_SLOTS][gridDim.x].
  // A block covers per_thread consecutive runs of ERR_BLOCK elements (thread t: element t of each run, in
  // run order), so that the single-block second pass has few partials to read on large grids.
  template <int S>
  __global__ __launch_bounds__(ERR_BLOCK) void k_error_norms(int NE, int per_thread, double hf, const double *__restrict__ u,
                                                             const double *__restrict__ v, const double *__restrict__ wq,
                                                             const double *__restrict__ wg, const double *__restrict__ c0,
                                                             const double *__restrict__ c1, double *__restrict__ partial)
  {
    __shared__ double red[ERR_BLOCK / 64][ERR_SLOTS];
    const size_t      nel = (size_t)NE * NE;
    double            l2[S], h1[S], linf[S], en = 0.0;
    for (int c = 0; c < S; ++c)
      l2[c] = h1[c] = linf[c] = 0.0;
    for (int run = 0; run < per_thread; ++run)
      {
        const size_t el = ((size_t)blockIdx.x * per_thread + run) * ERR_BLOCK + threadIdx.x;
        if (el >= nel)
          break;
        const int    ex = (int)(el % (size_t)NE), ey = (int)(el / (size_t)NE), np = NE + 1;
        const size_t n0 = (size_t)ey * np + ex, corner[4] = {n0, n0 + 1, n0 + np, n0 + np + 1};
        double       ed[S][4]; // nodal values of u - v at the corners (x fastest)
        for (int c = 0; c < S; ++c)
          for (int a = 0; a < 4; ++a)
            {
              const double uu = u ? u[corner[a] * S + c] : 0.0, vv = v ? v[corner[a] * S + c] : 0.0;
              ed[c][a]        = uu - vv;
            }
        double wv[S][4], wx[S][4], wy[S][4];
        if (wq)
          for (int c = 0; c < S; ++c)
            {
              load4(wq + ((size_t)c * nel + el) * 4, wv[c]);
              load4(wg + ((size_t)(2 * c) * nel + el) * 4, wx[c]);
              load4(wg + ((size_t)(2 * c + 1) * nel + el) * 4, wy[c]);
            }
        else
          for (int c = 0; c < S; ++c)
            for (int q = 0; q < 4; ++q)
              wv[c][q] = wx[c][q] = wy[c][q] = 0.0;
        double k0[4], k1[4] = {0.0, 0.0, 0.0, 0.0};
        load4(c0 + el * 4, k0);
        if (S == 2)
          load4(c1 + el * 4, k1);
        const double jxw = 0.25 * hf * hf, ih = 1.0 / hf;
        for (int q = 0; q < 4; ++q)
          {
            constexpr double g0 = 0.21132486540518711775, g1 = 0.78867513459481288225; // (1 -+ 1/sqrt 3)/2
            const double     xi = (q & 1) ? g1 : g0, eta = (q & 2) ? g1 : g0;
            // Q1 shape values and reference gradients at (xi, eta), corners (0,0) (1,0) (0,1) (1,1)
            const double N[4]  = {(1 - xi) * (1 - eta), xi * (1 - eta), (1 - xi) * eta, xi * eta};
            const double Gx[4] = {-(1 - eta), 1 - eta, -eta, eta};
            const double Gy[4] = {-(1 - xi), -xi, 1 - xi, xi};
            double       dx[S], dy[S];
            for (int c = 0; c < S; ++c)
              {
                double val = 0.0, gx = 0.0, gy = 0.0;
                for (int a = 0; a < 4; ++a)
                  {
                    val = fma(N[a], ed[c][a], val);
                    gx  = fma(Gx[a], ed[c][a], gx);
                    gy  = fma(Gy[a], ed[c][a], gy);
                  }
                val -= wv[c][q];
                dx[c]   = fma(gx, ih, -wx[c][q]);
                dy[c]   = fma(gy, ih, -wy[c][q]);
                l2[c]   = fma(val * val, jxw, l2[c]);
                h1[c]   = fma(dx[c] * dx[c] + dy[c] * dy[c], jxw, h1[c]);
                linf[c] = fmax(linf[c], fabs(val));
              }
            if (S == 1)
              en = fma(k0[q] * (dx[0] * dx[0] + dy[0] * dy[0]), jxw, en);
            else
              {
                // 2 mu eps(e):eps(e) + lambda (div e)^2 (Elasticity.h:245-254); field 0 = lambda, 1 = mu
                const double e00 = dx[0], e11 = dy[S - 1], e01 = 0.5 * (dy[0] + dx[S - 1]), dv = e00 + e11;
                en = fma(2.0 * k1[q] * (e00 * e00 + e11 * e11 + 2.0 * e01 * e01) + k0[q] * dv * dv, jxw, en);
              }
          }
      }
    double r[ERR_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < S; ++c)
      {
        r[c]     = l2[c];
        r[2 + c] = h1[c];
        r[4 + c] = linf[c];
      }
    r[6]             = en;
    const double tot = block_reduce<ERR_BLOCK>(r, red);
    if (threadIdx.x < ERR_SLOTS)
      partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = tot;
  }

  // out[k] = combination of partial[k][0 .. nblk): every thread walks its blocks in ascending order,
  // then the fixed wave/LDS tree of block_reduce (one block).  The loads of all slots and of UNROLL
  // consecutive blocks are issued together: a single block is bound by load latency, not bandwidth
  // (16384 partials per slot at NE = 2048).
  constexpr int COMBINE_BLOCK = 1024;
  __global__ __launch_bounds__(COMBINE_BLOCK) void k_error_combine(unsigned nblk, const double *__restrict__ partial,
                                                                   double *__restrict__ out)
  {
    constexpr int     UNROLL = 4;
    __shared__ double red[COMBINE_BLOCK / 64][ERR_SLOTS];
    double            r[ERR_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned b0 = threadIdx.x; b0 < nblk; b0 += UNROLL * COMBINE_BLOCK)
      {
        double p[UNROLL][ERR_SLOTS];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j)
          {
            const unsigned b = b0 + j * COMBINE_BLOCK;
#pragma unroll
            for (int k = 0; k < ERR_SLOTS; ++k)
              p[j][k] = b < nblk ? partial[(size_t)k * nblk + b] : 0.0;
          }
#pragma unroll
        for (int j = 0; j < UNROLL; ++j)
#pragma unroll
          for (int k = 0; k < ERR_SLOTS; ++k)
            r[k] = slot_is_max(k) ? fmax(r[k], p[j][k]) : r[k] + p[j][k];
      }
    const double tot = block_reduce<COMBINE_BLOCK>(r, red);
    if (threadIdx.x < ERR_SLOTS)
      out[threadIdx.x] = tot;
  }
} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_compute_error_norms(slod_handle *h, uint32_t problem, const double *d_u, const double *d_v,
                             const double *d_exact_qp, const double *d_exact_grad_qp, slod_error_norms *out,
                             void *hip_stream)
{
  if (!h || !out)
    return SLOD_ERR_ARGUMENT;
  if ((d_exact_qp == nullptr) != (d_exact_grad_qp == nullptr))
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_compute_error_norms: exact values and gradients go together");
  if ((reinterpret_cast<uintptr_t>(d_exact_qp) | reinterpret_cast<uintptr_t>(d_exact_grad_qp)) % 16)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_compute_error_norms: exact-solution arrays must be 16-byte aligned");
  if (problem >= (uint32_t)h->cfg.n_problems)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_compute_error_norms: problem out of range");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int s = h->cfg.spacedim;
  for (int f = 0; f < s; ++f)
    if (!h->coef_set[(size_t)problem * 2 + f])
      return slod_fail(h, SLOD_ERR_STATE, "slod_compute_error_norms: coefficient not set");
  // runs of ERR_BLOCK elements per block: 1 up to 2048 blocks, then as many as keep the partials at <= 2048
  // blocks (NE = 2048: 8).  A function of NE alone, so the summation order is fixed for the handle.
  const size_t   nel  = (size_t)h->NE * h->NE, runs = (nel + ERR_BLOCK - 1) / ERR_BLOCK;
  const int      per  = (int)std::min<size_t>(std::max<size_t>((runs + 2047) / 2048, 1), 64);
  const unsigned nblk = (unsigned)((runs + per - 1) / per);
  if (!h->d_err_ws)
    {
      // the handle's workspace (freed by slod_destroy): ERR_SLOTS partials per block, then the results
      const hipError_t e = hipMalloc((void **)&h->d_err_ws, ((size_t)nblk + 1) * ERR_SLOTS * sizeof(double));
      if (e != hipSuccess)
        {
          h->d_err_ws = nullptr;
          return slod_hip_fail(h, e, "slod_compute_error_norms: workspace");
        }
    }
  double       *partial = h->d_err_ws, *res = h->d_err_ws + (size_t)nblk * ERR_SLOTS;
  const size_t  cs = (size_t)problem * nel * 4;
  const double *c0 = h->d_coef[0] + cs, *c1 = s == 2 ? h->d_coef[1] + cs : nullptr;
  const double  hf = 1.0 / h->NE;
  if (s == 1)
    hipLaunchKernelGGL(k_error_norms<1>, dim3(nblk), dim3(ERR_BLOCK), 0, st, h->NE, per, hf, d_u, d_v, d_exact_qp,
                       d_exact_grad_qp, c0, c1, partial);
  else
    hipLaunchKernelGGL(k_error_norms<2>, dim3(nblk), dim3(ERR_BLOCK), 0, st, h->NE, per, hf, d_u, d_v, d_exact_qp,
                       d_exact_grad_qp, c0, c1, partial);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    {
      hipLaunchKernelGGL(k_error_combine, dim3(1), dim3(COMBINE_BLOCK), 0, st, nblk, partial, res);
      e = hipGetLastError();
    }
  double r[ERR_SLOTS];
  if (e == hipSuccess)
    e = hipMemcpyAsync(r, res, sizeof(r), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_compute_error_norms");
  *out = slod_error_norms();
  for (int c = 0; c < s; ++c)
    {
      out->l2[c]      = std::sqrt(r[c]);
      out->h1_semi[c] = std::sqrt(r[2 + c]);
      out->linf[c]    = r[4 + c];
    }
  out->energy = std::sqrt(r[6]);
  return SLOD_OK;
}

} // extern "C"
#pragma GCC visibility pop
