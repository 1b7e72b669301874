// The single-vector preconditioned CG of the global steps: scalars of the recurrence on the device (no host
// round trip per step), the kernels every such solve shares and the one host loop that drives them in bursts.
// Used by slod_lod_solve (slod_lod_system.hip: Jacobi on the block rows) and by the fine and coarse FEM solves
// (slod_fem.hip: multigrid or Jacobi on the stencil planes), which add their own init and product kernels.
#ifndef SLOD_CG_HIP_H
#define SLOD_CG_HIP_H
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>

namespace
{
  struct CgScalars
  {
    double rz, pAp, rz_new, rr, rhs2;
  };
  __global__ void k_cg_update_xr(int nrow, const double *pv, const double *Ap, const double *dinv, double *x, double *r,
                                 double *z, CgScalars *sc)
  {
    const int    i = blockIdx.x * 256 + threadIdx.x;
    const double alpha = sc->pAp != 0.0 ? sc->rz / sc->pAp : 0.0;
    double       a = 0.0, b = 0.0;
    if (i < nrow)
      {
        x[i] = fma(alpha, pv[i], x[i]);
        r[i] = fma(-alpha, Ap[i], r[i]);
        z[i] = dinv[i] * r[i];
        a    = r[i] * z[i];
        b    = r[i] * r[i];
      }
    for (int off = 32; off > 0; off >>= 1)
      {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
      }
    if ((threadIdx.x & 63) == 0)
      {
        atomicAdd(&sc->rz_new, a);
        atomicAdd(&sc->rr, b);
      }
  }
  __global__ void k_cg_update_p(int nrow, const double *z, double *pv, const CgScalars *sc)
  {
    const int    i = blockIdx.x * 256 + threadIdx.x;
    const double beta = sc->rz != 0.0 ? sc->rz_new / sc->rz : 0.0;
    if (i < nrow)
      pv[i] = fma(beta, pv[i], z[i]);
  }
  __global__ void k_cg_rotate(CgScalars *sc)
  {
    sc->rz     = sc->rz_new;
    sc->rz_new = 0.0;
    sc->pAp    = 0.0;
    sc->rr     = 0.0;
  }
  // CG pieces around a general preconditioner: x += alpha p, r -= alpha Ap, rr; then rz_new = r.z
  __global__ void k_pcg_update_xr(int nrow, const double *pv, const double *Ap, double *x, double *r, CgScalars *sc)
  {
    const int    i = blockIdx.x * 256 + threadIdx.x;
    const double alpha = sc->pAp != 0.0 ? sc->rz / sc->pAp : 0.0;
    double       b = 0.0;
    if (i < nrow)
      {
        x[i] = fma(alpha, pv[i], x[i]);
        r[i] = fma(-alpha, Ap[i], r[i]);
        b    = r[i] * r[i];
      }
    for (int off = 32; off > 0; off >>= 1)
      b += __shfl_xor(b, off, 64);
    if ((threadIdx.x & 63) == 0)
      atomicAdd(&sc->rr, b);
  }
  __global__ void k_pcg_dot_rz(int nrow, const double *r, const double *z, CgScalars *sc, int first)
  {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double    a = i < nrow ? r[i] * z[i] : 0.0;
    for (int off = 32; off > 0; off >>= 1)
      a += __shfl_xor(a, off, 64);
    if ((threadIdx.x & 63) == 0)
      atomicAdd(first ? &sc->rz : &sc->rz_new, a);
  }
  __global__ void k_copy(int n, const double *src, double *dst)
  {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
      dst[i] = src[i];
  }

  // The iterations of a solve whose init kernels the caller has enqueued on st: they left x = 0, r, z, p and,
  // in the zeroed *sc, rz = r.z and rhs2 = rr = r.r.  step() enqueues one CG step (the product with its p.Ap,
  // the update of x and r with its r.r, the preconditioner with the new r.z in rz_new, the update of p); the
  // driver puts k_cg_rotate between the steps and checks r.r <= rel_tol^2 rhs2 on the host once per burst, so
  // *it is a multiple of burst or max_iterations.  The stream is idle on return.  *rel_residual (may be
  // null) is sqrt(r.r / rhs2) of the last step, 0 for a zero right-hand side.
  template <typename Step>
  hipError_t slod_cg_drive(hipStream_t st, CgScalars *sc, int burst_len, int max_iterations, double rel_tol, Step step, int *it,
                           double *rel_residual)
  {
    CgScalars  hs;
    hipError_t e = hipMemcpyAsync(&hs, sc, sizeof(hs), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
      e = hipStreamSynchronize(st);
    const double rhs2 = hs.rhs2;
    // The init kernel added the same per-wave partials to rhs2 and to rr, but by two atomicAdds each, whose order over
    // the waves is not fixed: the two sums can differ in the last bits.  The initial residual is the right-hand side, so
    // it takes the one sum; clear the per-iteration sums
    double rr = rhs2;
    if (e == hipSuccess)
      {
        hs.rr = 0.0;
        hs.pAp = 0.0;
        hs.rz_new = 0.0;
        e = hipMemcpyAsync(sc, &hs, sizeof(hs), hipMemcpyHostToDevice, st);
      }
    *it = 0;
    while (e == hipSuccess && *it < max_iterations && rhs2 > 0.0 && rr > rel_tol * rel_tol * rhs2)
      {
        // a burst of iterations per convergence check: the scalars stay on the device in between
        const int burst = std::min(burst_len, max_iterations - *it);
        for (int b = 0; b < burst; ++b)
          {
            step();
            if (b + 1 < burst)
              hipLaunchKernelGGL(k_cg_rotate, dim3(1), dim3(1), 0, st, sc);
          }
        *it += burst;
        e = hipMemcpyAsync(&hs, sc, sizeof(hs), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
          e = hipStreamSynchronize(st);
        rr = hs.rr;
        if (e == hipSuccess)
          hipLaunchKernelGGL(k_cg_rotate, dim3(1), dim3(1), 0, st, sc);
      }
    if (e == hipSuccess)
      e = hipStreamSynchronize(st);
    if (rel_residual)
      *rel_residual = rhs2 > 0.0 ? std::sqrt(rr / rhs2) : 0.0;
    return e;
  }
} // namespace
#endif
