// The reference problems the LOD solution is compared with, on the stencil planes of k_assemble: the fine
// FEM problem on the global fine grid and the coarse FEM(H) problem (assemble_and_solve_fem_problem,
// LOD.cc:1004-1237), both solved by the CG of slod_cg.hip.h, multigrid-preconditioned where that applies.
// Nodal fields are [(NE+1)^2][s]; Dirichlet nodes (every side of the domain) are identity rows with value 0.
#include "slod_host.h"
#include "slod_cg.hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace
{
  // ---- fine FEM reference problem on the global fine grid (assemble_and_solve_fem_problem,
  // LOD.cc:1004-1094): load vector of assemble_stiffness (Diffusion.h:149-193) and a matrix-free
  // Jacobi-CG on the 9-point block stencil planes of k_assemble (whole domain = one "patch").
  // Dirichlet nodes (every side of the domain, LOD.cc:1021) are identity rows with value 0.
  __global__ void k_fem_rhs(int NE, int s, double h2q, const double *f_qp, double *rhs)
  {
    const int np = NE + 1, node = blockIdx.x * 256 + threadIdx.x;
    if (node >= np * np)
      return;
    const int  ix = node % np, iy = node / np;
    const bool bnd = ix == 0 || iy == 0 || ix == NE || iy == NE;
    for (int c = 0; c < s; ++c)
      {
        double acc = 0.0;
        if (!bnd)
          for (int ay = 0; ay < 2; ++ay)
            for (int ax = 0; ax < 2; ++ax)
              {
                const int    ex = ix - ax, ey = iy - ay; // element that has this node as its corner (ax, ay)
                const size_t ge = ((size_t)ey * NE + ex) * 4;
                for (int q = 0; q < 4; ++q)
                  {
                    constexpr double g0 = 0.21132486540518711775, g1 = 0.78867513459481288225; // (1 -+ 1/sqrt 3)/2
                    const double     xi = (q & 1) ? g1 : g0, eta = (q & 2) ? g1 : g0;
                    const double     N  = (ax ? xi : 1.0 - xi) * (ay ? eta : 1.0 - eta);
                    acc += N * (f_qp ? f_qp[(size_t)c * NE * NE * 4 + ge + q] : 1.0) * h2q;
                  }
              }
        rhs[(size_t)node * s + c] = acc;
      }
  }
  // y = A x on the interior nodes (x, y: [(NE+1)^2][s]); boundary rows: y = x.  Also accumulates
  // x.y into sc->pAp.  st: planes [(dir*s + a)*s + b][nn], dir = (dy+1)*3 + dx+1.
  __global__ void k_fem_spmv_dot(int NE, int s, const double *st, const double *x, double *y, CgScalars *sc)
  {
    const int    np = NE + 1, nn = np * np, node = blockIdx.x * 256 + threadIdx.x;
    double       part = 0.0;
    if (node < nn)
      {
        const int  ix = node % np, iy = node / np;
        const bool bnd = ix == 0 || iy == 0 || ix == NE || iy == NE;
        for (int a = 0; a < s; ++a)
          {
            double acc = 0.0;
            if (bnd)
              acc = x[(size_t)node * s + a];
            else
              for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                  {
                    const int jx = ix + dx, jy = iy + dy;
                    if (jx == 0 || jy == 0 || jx == NE || jy == NE)
                      continue; // constrained neighbour: value 0
                    const int dir = (dy + 1) * 3 + dx + 1, nb = jx + jy * np;
                    for (int b = 0; b < s; ++b)
                      acc = fma(st[(size_t)((dir * s + a) * s + b) * nn + node], x[(size_t)nb * s + b], acc);
                  }
            y[(size_t)node * s + a] = acc;
            part += acc * x[(size_t)node * s + a];
          }
      }
    for (int off = 32; off > 0; off >>= 1)
      part += __shfl_xor(part, off, 64);
    if ((threadIdx.x & 63) == 0 && part != 0.0)
      atomicAdd(&sc->pAp, part);
  }
  __global__ void k_fem_init(int NE, int s, const double *st, const double *rhs, double *x, double *r, double *z, double *pv,
                             double *dinv, CgScalars *sc)
  {
    const int np = NE + 1, nn = np * np, node = blockIdx.x * 256 + threadIdx.x;
    double    a = 0.0, b = 0.0;
    if (node < nn)
      {
        const int  ix = node % np, iy = node / np;
        const bool bnd = ix == 0 || iy == 0 || ix == NE || iy == NE;
        for (int c = 0; c < s; ++c)
          {
            const size_t i    = (size_t)node * s + c;
            const double diag = bnd ? 1.0 : st[(size_t)((4 * s + c) * s + c) * nn + node];
            const double f    = bnd ? 0.0 : rhs[i];
            dinv[i]           = diag != 0.0 ? 1.0 / diag : 1.0;
            x[i]              = 0.0;
            r[i]              = f;
            z[i]              = dinv[i] * f;
            pv[i]             = z[i];
            a += f * z[i];
            b += f * f;
          }
      }
    for (int off = 32; off > 0; off >>= 1)
      {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
      }
    if ((threadIdx.x & 63) == 0)
      {
        atomicAdd(&sc->rz, a);
        atomicAdd(&sc->rhs2, b);
        atomicAdd(&sc->rr, b);
      }
  }

  // ---- geometric multigrid V-cycle on the 9-point block stencil planes: the preconditioner of the
  // fine FEM reference solve (the reference uses CG + AMG, LOD.cc:1070-1075).  Levels halve the grid
  // while the number of elements per side is even; bilinear interpolation P, restriction P^T, Galerkin
  // coarse operators P^T A P (again 9-point stencils), damped-Jacobi smoothing with the same number
  // of sweeps before and after the coarse correction (a symmetric preconditioner).  It is positive definite
  // because every level damps with omega_l = min(0.8, 1.6 / ||D_l^-1 A_l||_inf), D_l the diagonal (s = 1) or the
  // 2 x 2 node blocks (s = 2): omega_l lambda_max(D_l^-1 A_l) <= 1.6 < 2 by the row sums of the level's own
  // planes (k_mg_rowsum).  Nothing else bounds lambda_max: Galerkin levels of a high-contrast field exceed the
  // 1.5 of a Q1 Laplacian (1.63 scalar, 3.2 for elasticity at contrast 1e4), and a constant 0.8 then makes the
  // V-cycle indefinite.  Dirichlet nodes (all four sides) carry 0 on every level and are no unknowns.
  __device__ __forceinline__ double mg_w(int f, int c) // 1-D bilinear weight of coarse node c at fine node f
  {
    const int dlt = f - 2 * c;
    return dlt == 0 ? 1.0 : ((dlt == 1 || dlt == -1) ? 0.5 : 0.0);
  }
  // coarse planes from fine planes: one thread per coarse node
  __global__ void k_mg_galerkin(int Nf, int s, const double *stf, double *stc)
  {
    const int Nc = Nf / 2, npc = Nc + 1, nnc = npc * npc, npf = Nf + 1, nnf = npf * npf;
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= nnc)
      return;
    const int X = node % npc, Y = node / npc;
    double    acc[9][2][2];
    for (int q = 0; q < 9; ++q)
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
          acc[q][a][b] = 0.0;
    const bool bnd = X == 0 || Y == 0 || X == Nc || Y == Nc;
    if (!bnd)
      for (int ay = -1; ay <= 1; ++ay)
        for (int ax = -1; ax <= 1; ++ax)
          {
            const int ix = 2 * X + ax, iy = 2 * Y + ay; // fine node in the support of the coarse hat (interior)
            if (ix <= 0 || iy <= 0 || ix >= Nf || iy >= Nf)
              continue;
            const double wi = mg_w(ix, X) * mg_w(iy, Y);
            const int    fn = ix + iy * npf;
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx)
                {
                  const int jx = ix + dx, jy = iy + dy;
                  if (jx <= 0 || jy <= 0 || jx >= Nf || jy >= Nf)
                    continue; // constrained fine neighbour
                  const int dir = (dy + 1) * 3 + dx + 1;
                  for (int DY = -1; DY <= 1; ++DY)
                    for (int DX = -1; DX <= 1; ++DX)
                      {
                        const double wj = mg_w(jx, X + DX) * mg_w(jy, Y + DY);
                        if (wj == 0.0)
                          continue;
                        const int q = (DY + 1) * 3 + DX + 1;
                        for (int a = 0; a < s; ++a)
                          for (int b = 0; b < s; ++b)
                            acc[q][a][b] = fma(wi * wj, stf[(size_t)((dir * s + a) * s + b) * nnf + fn], acc[q][a][b]);
                      }
                }
          }
    for (int q = 0; q < 9; ++q)
      for (int a = 0; a < s; ++a)
        for (int b = 0; b < s; ++b)
          stc[(size_t)((q * s + a) * s + b) * nnc + node] = acc[q][a][b];
  }
  // (A x)(node, a) on the interior, constrained neighbours skipped
  __device__ __forceinline__ double mg_apply(int N, int s, const double *st, const double *x, int ix, int iy, int a)
  {
    const int np = N + 1, nn = np * np, node = ix + iy * np;
    double    acc = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx)
        {
          const int jx = ix + dx, jy = iy + dy;
          if (jx == 0 || jy == 0 || jx == N || jy == N)
            continue;
          const int dir = (dy + 1) * 3 + dx + 1, nb = jx + jy * np;
          for (int b = 0; b < s; ++b)
            acc = fma(st[(size_t)((dir * s + a) * s + b) * nn + node], x[(size_t)nb * s + b], acc);
        }
    return acc;
  }
  // *out = max(*out, ||D^-1 A||_inf) over the interior rows, D the s x s node blocks: one thread per node.  A maximum
  // of non-negative doubles is the maximum of their bit patterns and does not depend on the order of the atomics.
  __global__ void k_mg_rowsum(int N, int s, const double *st, unsigned long long *out)
  {
    const int np = N + 1, nn = np * np, node = blockIdx.x * 256 + threadIdx.x;
    double    m = 0.0;
    if (node < nn)
      {
        const int ix = node % np, iy = node / np;
        if (!(ix == 0 || iy == 0 || ix == N || iy == N))
          {
            const double d00 = st[(size_t)((4 * s + 0) * s + 0) * nn + node];
            double       d01 = 0.0, d10 = 0.0, d11 = 1.0;
            if (s == 2)
              {
                d01 = st[(size_t)((4 * s + 0) * s + 1) * nn + node];
                d10 = st[(size_t)((4 * s + 1) * s + 0) * nn + node];
                d11 = st[(size_t)((4 * s + 1) * s + 1) * nn + node];
              }
            const double det = d00 * d11 - d01 * d10;
            double       sum[2] = {0.0, 0.0};
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx)
                {
                  const int jx = ix + dx, jy = iy + dy;
                  if (jx == 0 || jy == 0 || jx == N || jy == N)
                    continue; // constrained neighbour: no column
                  const int dir = (dy + 1) * 3 + dx + 1;
                  for (int b = 0; b < s; ++b)
                    {
                      const double a0 = st[(size_t)((dir * s + 0) * s + b) * nn + node];
                      const double a1 = s == 2 ? st[(size_t)((dir * s + 1) * s + b) * nn + node] : 0.0;
                      sum[0] += fabs((d11 * a0 - d01 * a1) / det);
                      sum[1] += fabs((d00 * a1 - d10 * a0) / det);
                    }
                }
            m = fmax(sum[0], sum[1]);
          }
      }
    for (int off = 32; off > 0; off >>= 1)
      m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0)
      atomicMax(out, (unsigned long long)__double_as_longlong(m));
  }
  // xo = xi + omega D^-1 (b - A xi)   (zero_in: xi = 0); omega = min(0.8, 1.6 / *rowsum), or 1 without a row sum
  __global__ void k_mg_smooth(int N, int s, const double *st, const double *b, const double *xi, double *xo,
                              const double *rowsum, int zero_in)
  {
    const int np = N + 1, nn = np * np, node = blockIdx.x * 256 + threadIdx.x;
    if (node >= nn)
      return;
    const double omega = rowsum ? fmin(0.8, 1.6 / *rowsum) : 1.0;
    const int  ix = node % np, iy = node / np;
    const bool bnd = ix == 0 || iy == 0 || ix == N || iy == N;
    double     r[2] = {0.0, 0.0}, v[2] = {0.0, 0.0};
    if (!bnd)
      {
        for (int a = 0; a < s; ++a)
          r[a] = b[(size_t)node * s + a] - (zero_in ? 0.0 : mg_apply(N, s, st, xi, ix, iy, a));
        // block Jacobi: the s x s diagonal block of the node (vector problems: point Jacobi stalls where lambda >> mu)
        const double d00 = st[(size_t)((4 * s + 0) * s + 0) * nn + node];
        if (s == 1)
          v[0] = r[0] / d00;
        else
          {
            const double d01 = st[(size_t)((4 * s + 0) * s + 1) * nn + node], d10 = st[(size_t)((4 * s + 1) * s + 0) * nn + node],
                         d11 = st[(size_t)((4 * s + 1) * s + 1) * nn + node];
            const double det = d00 * d11 - d01 * d10;
            v[0]             = (d11 * r[0] - d01 * r[1]) / det;
            v[1]             = (d00 * r[1] - d10 * r[0]) / det;
          }
      }
    for (int a = 0; a < s; ++a)
      {
        const size_t i = (size_t)node * s + a;
        xo[i]          = bnd ? 0.0 : (zero_in ? 0.0 : xi[i]) + omega * v[a];
      }
  }
  // bc = P^T (b - A x): one thread per coarse node gathers its 3 x 3 fine residuals
  __global__ void k_mg_restrict(int Nf, int s, const double *st, const double *b, const double *x, double *bc)
  {
    const int Nc = Nf / 2, npc = Nc + 1, nnc = npc * npc, npf = Nf + 1;
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= nnc)
      return;
    const int  X = node % npc, Y = node / npc;
    const bool bnd = X == 0 || Y == 0 || X == Nc || Y == Nc;
    for (int a = 0; a < s; ++a)
      {
        double acc = 0.0;
        if (!bnd)
          for (int ay = -1; ay <= 1; ++ay)
            for (int ax = -1; ax <= 1; ++ax)
              {
                const int ix = 2 * X + ax, iy = 2 * Y + ay;
                if (ix <= 0 || iy <= 0 || ix >= Nf || iy >= Nf)
                  continue;
                const double r = b[(size_t)(ix + iy * npf) * s + a] - mg_apply(Nf, s, st, x, ix, iy, a);
                acc            = fma(mg_w(ix, X) * mg_w(iy, Y), r, acc);
              }
        bc[(size_t)node * s + a] = acc;
      }
  }
  // x += P xc
  __global__ void k_mg_prolong_add(int Nf, int s, const double *xc, double *x)
  {
    const int Nc = Nf / 2, npc = Nc + 1, npf = Nf + 1, nnf = npf * npf;
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= nnf)
      return;
    const int ix = node % npf, iy = node / npf;
    if (ix == 0 || iy == 0 || ix == Nf || iy == Nf)
      return;
    for (int a = 0; a < s; ++a)
      {
        double acc = 0.0;
        for (int Y = iy / 2; Y <= (iy + 1) / 2; ++Y)
          for (int X = ix / 2; X <= (ix + 1) / 2; ++X)
            acc = fma(mg_w(ix, X) * mg_w(iy, Y), xc[(size_t)(X + Y * npc) * s + a], acc);
        x[(size_t)node * s + a] += acc;
      }
  }
  __global__ void k_pcg_init(int NE, int s, const double *rhs, double *x, double *r, CgScalars *sc)
  {
    const int np = NE + 1, nn = np * np, node = blockIdx.x * 256 + threadIdx.x;
    double    b = 0.0;
    if (node < nn)
      {
        const int  ix = node % np, iy = node / np;
        const bool bnd = ix == 0 || iy == 0 || ix == NE || iy == NE;
        for (int c = 0; c < s; ++c)
          {
            const size_t i = (size_t)node * s + c;
            const double f = bnd ? 0.0 : rhs[i];
            x[i]           = 0.0;
            r[i]           = f;
            b += f * f;
          }
      }
    for (int off = 32; off > 0; off >>= 1)
      b += __shfl_xor(b, off, 64);
    if ((threadIdx.x & 63) == 0)
      {
        atomicAdd(&sc->rhs2, b);
        atomicAdd(&sc->rr, b);
      }
  }

  // ---- coarse FEM(H) reference problem (the coarse part of assemble_and_solve_fem_problem,
  // LOD.cc:1103-1237): Q1 on the coarse mesh, the coefficient at the 2 x 2 Gauss points of every coarse
  // cell (assemble_stiffness_coarse, Diffusion.h:210-305, Elasticity.h:304ff).  Stiffness, load vector and
  // solve are the fine-grid kernels with NE := N; new are only the sampling and the interpolation back.
  //
  // Where the coarse Gauss abscissa (C + g[k]) H falls in the fine grid, per axis: fine element C n + off[k],
  // quadrature slot slot[k] of that element (the stored fine field read as piecewise constant on the
  // quadrants of the fine elements).  Computed once on the host from n (coarse_sample_rule): no per-thread
  // floating-point floor decides an index.
  struct CoarseSampleRule
  {
    int32_t off[2], slot[2];
  };
  // out [N][N][4] (q = q0 + 2 q1, the layout of a fine field with NE -> N) from fine [NE][NE][4]
  __global__ void k_coarse_sample(int N, int n, const CoarseSampleRule R, const double *fine, double *out)
  {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * N * 4)
      return;
    const int    q0 = (int)(i & 1), q1 = (int)((i >> 1) & 1);
    const size_t cell = i >> 2;
    const int    Cx = (int)(cell % (size_t)N), Cy = (int)(cell / (size_t)N), NE = N * n;
    const int    ex = Cx * n + R.off[q0], ey = Cy * n + R.off[q1]; // off <= n - 1: inside the coarse cell
    out[i]          = fine[((size_t)ey * NE + ex) * 4 + R.slot[q0] + 2 * R.slot[q1]];
  }
  // fem_coarse_solution_interpolated (FETools::interpolate, LOD.cc:1201-1204): bilinear interpolant of the
  // coarse nodal field [(N+1)^2][s] at every fine node, [(NE+1)^2][s].  One thread per fine node, blockIdx.y
  // walks the node rows (no division by the row length; consecutive threads store consecutive nodes).  The
  // weights are the integers (n - rx, rx) x (n - ry, ry) over n^2, so a field that is exactly representable
  // sees one rounding (the division); a fine node on a coarse node copies the value bit for bit.
  __global__ void k_coarse_prolong(int N, int n, int s, const double *coarse, double *fine)
  {
    const int NE = N * n, np = NE + 1, npc = N + 1;
    const int ix = blockIdx.x * 256 + threadIdx.x;
    if (ix >= np)
      return;
    const int Cx = ix / n < N ? ix / n : N - 1, rx = ix - Cx * n; // the last node line: cell N - 1, rx = n
    for (int iy = blockIdx.y; iy < np; iy += gridDim.y)
      {
        const int    Cy = iy / n < N ? iy / n : N - 1, ry = iy - Cy * n; // rx, ry in [0, n]
        const size_t node = (size_t)iy * np + ix, c00 = (size_t)Cx + (size_t)Cy * npc;
        if ((rx == 0 || rx == n) && (ry == 0 || ry == n))
          {
            const size_t src = c00 + (rx ? 1 : 0) + (ry ? (size_t)npc : 0);
            for (int c = 0; c < s; ++c)
              fine[node * s + c] = coarse[src * s + c];
            continue;
          }
        const double w00 = (double)((n - rx) * (n - ry)), w10 = (double)(rx * (n - ry)), w01 = (double)((n - rx) * ry),
                     w11 = (double)(rx * ry), nn = (double)n * (double)n;
        for (int c = 0; c < s; ++c)
          {
            // (a weight of 0 still reads its corner: every corner is a node of the coarse grid)
            const double v = w00 * coarse[c00 * s + c] + w10 * coarse[(c00 + 1) * s + c] + w01 * coarse[(c00 + npc) * s + c] +
                             w11 * coarse[(c00 + npc + 1) * s + c];
            fine[node * s + c] = v / nn;
          }
      }
  }

  // Multigrid hierarchy on the stencil planes (level 0 = the fine grid, whose planes the caller owns): planes,
  // right-hand side and two iterates per level in one allocation, Galerkin coarse operators built by build().
  struct MgHierarchy
  {
    struct Level
    {
      int     N;
      double *st, *b, *x, *y, *rowsum; // rowsum: ||D^-1 A||_inf of the level (k_mg_rowsum), on the device
    };
    hipStream_t        st;
    int                s;
    std::vector<Level> lev;
    SlodDevBuf<double> mem;
    hipError_t build(int NE, double *planes)
    {
      size_t need = 0;
      for (int N = NE; ; N /= 2)
        {
          const size_t nnl = (size_t)(N + 1) * (N + 1);
          need += (N == NE ? 0 : (size_t)9 * s * s * nnl) + 3 * nnl * s;
          lev.push_back({N, nullptr, nullptr, nullptr, nullptr, nullptr});
          if (N % 2 || N / 2 < 2)
            break;
        }
      hipError_t e = mem.alloc(need + lev.size());
      double    *q = mem.get();
      if (e == hipSuccess)
        e = hipMemsetAsync(q + need, 0, lev.size() * sizeof(double), st);
      for (size_t l = 0; l < lev.size() && e == hipSuccess; ++l)
        {
          const size_t nnl = (size_t)(lev[l].N + 1) * (lev[l].N + 1);
          lev[l].st = l == 0 ? planes : q;
          q += l == 0 ? 0 : (size_t)9 * s * s * nnl;
          lev[l].b = q;
          lev[l].x = q + nnl * s;
          lev[l].y = q + 2 * nnl * s;
          q += 3 * nnl * s;
          if (l > 0)
            hipLaunchKernelGGL(k_mg_galerkin, dim3((unsigned)((nnl + 255) / 256)), dim3(256), 0, st, lev[l - 1].N, s, lev[l - 1].st,
                               lev[l].st);
          lev[l].rowsum = mem.get() + need + l;
          hipLaunchKernelGGL(k_mg_rowsum, dim3((unsigned)((nnl + 255) / 256)), dim3(256), 0, st, lev[l].N, s, lev[l].st,
                             reinterpret_cast<unsigned long long *>(lev[l].rowsum));
        }
      return e == hipSuccess ? hipGetLastError() : e;
    }

    // z = V-cycle(r): V(2,2), damped (block) Jacobi with the omega_l of the level; the coarsest level by a fixed, even
    // number of sweeps, undamped when it has one interior node (N = 2: the first sweep solves it)
    void cycle(const double *rin, double *zout) const
    {
      const int nu = 2;
      for (size_t l = 0; l < lev.size(); ++l)
        {
          const Level  &L = lev[l];
          const int     nnl = (L.N + 1) * (L.N + 1), nb = (nnl + 255) / 256;
          const double *bl = l == 0 ? rin : L.b;
          const bool    last = l + 1 == lev.size();
          const int     sweeps = last ? (L.N <= 2 ? 2 : 40) : nu;
          double       *xi = L.x, *xo = L.y;
          for (int k = 0; k < sweeps; ++k)
            {
              hipLaunchKernelGGL(k_mg_smooth, dim3(nb), dim3(256), 0, st, L.N, s, L.st, bl, xi, xo, L.N <= 2 ? nullptr : L.rowsum,
                                 k == 0 ? 1 : 0);
              std::swap(xi, xo);
            }
          // sweeps is even: the current iterate is back in L.x
          if (!last)
            {
              const int nnc = (L.N / 2 + 1) * (L.N / 2 + 1);
              hipLaunchKernelGGL(k_mg_restrict, dim3((nnc + 255) / 256), dim3(256), 0, st, L.N, s, L.st, bl, L.x, lev[l + 1].b);
            }
        }
      for (size_t l = lev.size() - 1; l-- > 0;)
        {
          const Level  &L = lev[l];
          const int     nnl = (L.N + 1) * (L.N + 1), nb = (nnl + 255) / 256;
          const double *bl = l == 0 ? rin : L.b;
          hipLaunchKernelGGL(k_mg_prolong_add, dim3(nb), dim3(256), 0, st, L.N, s, lev[l + 1].x, L.x);
          double *xi = L.x, *xo = L.y;
          for (int k = 0; k < nu; ++k)
            {
              hipLaunchKernelGGL(k_mg_smooth, dim3(nb), dim3(256), 0, st, L.N, s, L.st, bl, xi, xo, L.rowsum, 0);
              std::swap(xi, xo);
            }
        }
      const size_t nrow = (size_t)(lev[0].N + 1) * (lev[0].N + 1) * s;
      hipLaunchKernelGGL(k_copy, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, st, (int)nrow, lev[0].x, zout);
    }
  };
} // namespace

// position of the two coarse Gauss abscissae of one axis in the fine grid (see CoarseSampleRule); n g is
// irrational, so the point never sits on an element edge or on a quadrant boundary
static CoarseSampleRule coarse_sample_rule(int n)
{
  const double     g[2] = {0.21132486540518711775, 0.78867513459481288225}; // (1 -+ 1/sqrt 3)/2
  CoarseSampleRule R;
  for (int k = 0; k < 2; ++k)
    {
      const double t = n * g[k];
      R.off[k]       = (int32_t)std::floor(t);
      R.slot[k]      = t - std::floor(t) >= 0.5 ? 1 : 0;
    }
  return R;
}

// The Q1 problem on an NE x NE grid of the unit square, on the handle's stream: stencil planes of k_assemble
// from the coefficient fields c0, c1 ([NE][NE][4] each, c1 for spacedim 2 only), then the CG bursts with
// device scalars, multigrid-preconditioned where that applies.  slod_fem_solve calls it with the fine grid
// and the stored field of a problem, slod_coarse_fem_solve with the coarse grid and the sampled field.
// Returns the iteration count or a negative slod_status (`who` names the caller in the error text).
static int fem_solve_grid(slod_handle *h, const char *who, int NE, const double *c0, const double *c1, const double *d_fine_rhs,
                          double *d_fine_u, double rel_tol, int max_iterations, double *rel_residual)
{
  const int                 s = h->cfg.spacedim;
  hipStream_t               st = h->stream;
  const int                 nn = (NE + 1) * (NE + 1), nblk = (nn + 255) / 256;
  const size_t              nrow = (size_t)nn * s;
  const int                 nb1 = (int)((nrow + 255) / 256);
  SlodDevBuf<double>        planes_buf, work;
  SlodDevBuf<SlodPatchDesc> d_desc;
  SlodDevBuf<CgScalars>     sc_buf;
  hipError_t                e = planes_buf.alloc((size_t)9 * s * s * nn);
  if (e == hipSuccess)
    e = work.alloc(5 * nrow);
  if (e == hipSuccess)
    e = d_desc.alloc(1);
  if (e == hipSuccess)
    e = sc_buf.alloc(1);
  double *const    planes = planes_buf.get();
  CgScalars *const sc = sc_buf.get();
  if (e == hipSuccess)
    e = hipMemsetAsync(sc, 0, sizeof(CgScalars), st);
  if (e == hipSuccess)
    {
      // the whole domain as one patch of k_assemble: NE x NE elements at the origin
      SlodPatchDesc d;
      std::memset(&d, 0, sizeof(d));
      d.nx   = NE;
      d.ny   = NE;
      d.prob = 0; // c0, c1 point at the field itself
      e      = hipMemcpyAsync(d_desc.get(), &d, sizeof(d), hipMemcpyHostToDevice, st);
      SlodKernelArgs a;
      std::memset(&a, 0, sizeof(a));
      a.desc        = d_desc.get();
      a.coef0       = c0;
      a.coef1       = c1;
      a.coef_stride = (size_t)NE * NE * 4;
      a.NE          = NE;
      a.n_sub       = h->cfg.n_subdivisions;
      a.st          = planes;
      a.st_stride   = (size_t)9 * s * s * nn;
      a.nn_max      = nn;
      if (e == hipSuccess)
        e = slod_launch_assemble(s, a, 1, st);
    }
  const char *pc_env = std::getenv("SLOD_FEM_PRECOND");
  // (Scalar problems take the V-cycle, vector problems keep Jacobi unless SLOD_FEM_PRECOND=mg asks for it.  The
  // 4500 against 1376 iterations once measured for elasticity at contrast 1e4 on the 65^2 grid were those of an
  // indefinite preconditioner: with a constant omega = 0.8 and lambda_max(D^-1 A) up to 3.2 on the block-Jacobi
  // levels, 0.8 lambda_max > 2.  With the per-level omega_l of MgHierarchy the same solve takes 104 iterations
  // against Jacobi's 1376 (tests/test_gpu_lod_system.py).  Which of the two is faster for vector problems is a
  // question of time per iteration and has not been decided: the default is unchanged.)
  const bool  want_mg = pc_env ? !strcmp(pc_env, "mg") : s == 1;
  const bool  use_mg = want_mg && NE >= 4 && NE % 2 == 0;
  MgHierarchy mg{st, s};
  if (e == hipSuccess && use_mg)
    e = mg.build(NE, planes);
  double *r = work.get(), *z = r + nrow, *pv = r + 2 * nrow, *Ap = r + 3 * nrow, *dinv = r + 4 * nrow;
  int     it = 0;
  // the driver synchronises st before it returns: every buffer of this function is idle when it is freed
  if (e == hipSuccess && use_mg)
    {
      hipLaunchKernelGGL(k_pcg_init, dim3(nblk), dim3(256), 0, st, NE, s, d_fine_rhs, d_fine_u, r, sc);
      mg.cycle(r, z);
      hipLaunchKernelGGL(k_pcg_dot_rz, dim3(nb1), dim3(256), 0, st, (int)nrow, r, z, sc, 1);
      hipLaunchKernelGGL(k_copy, dim3(nb1), dim3(256), 0, st, (int)nrow, z, pv);
      const auto step = [&] {
        hipLaunchKernelGGL(k_fem_spmv_dot, dim3(nblk), dim3(256), 0, st, NE, s, planes, pv, Ap, sc);
        hipLaunchKernelGGL(k_pcg_update_xr, dim3(nb1), dim3(256), 0, st, (int)nrow, pv, Ap, d_fine_u, r, sc);
        mg.cycle(r, z);
        hipLaunchKernelGGL(k_pcg_dot_rz, dim3(nb1), dim3(256), 0, st, (int)nrow, r, z, sc, 0);
        hipLaunchKernelGGL(k_cg_update_p, dim3(nb1), dim3(256), 0, st, (int)nrow, z, pv, sc);
      };
      e = slod_cg_drive(st, sc, 4, max_iterations, rel_tol, step, &it, rel_residual);
    }
  else if (e == hipSuccess)
    {
      hipLaunchKernelGGL(k_fem_init, dim3(nblk), dim3(256), 0, st, NE, s, planes, d_fine_rhs, d_fine_u, r, z, pv, dinv, sc);
      const auto step = [&] {
        hipLaunchKernelGGL(k_fem_spmv_dot, dim3(nblk), dim3(256), 0, st, NE, s, planes, pv, Ap, sc);
        hipLaunchKernelGGL(k_cg_update_xr, dim3(nb1), dim3(256), 0, st, (int)nrow, pv, Ap, dinv, d_fine_u, r, z, sc);
        hipLaunchKernelGGL(k_cg_update_p, dim3(nb1), dim3(256), 0, st, (int)nrow, z, pv, sc);
      };
      e = slod_cg_drive(st, sc, 32, max_iterations, rel_tol, step, &it, rel_residual);
    }
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who);
  return it;
}

#pragma GCC visibility push(default)
extern "C" {

int slod_fem_rhs(slod_handle *h, const double *d_f_qp, double *d_fine_rhs, void *hip_stream)
{
  if (!h || !d_fine_rhs)
    return SLOD_ERR_ARGUMENT;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int    nn = (h->NE + 1) * (h->NE + 1);
  const double hf = 1.0 / h->NE;
  hipLaunchKernelGGL(k_fem_rhs, dim3((nn + 255) / 256), dim3(256), 0, st, h->NE, h->cfg.spacedim, hf * hf * 0.25, d_f_qp,
                     d_fine_rhs);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_fem_rhs");
}

int slod_fem_solve(slod_handle *h, uint32_t problem, const double *d_fine_rhs, double *d_fine_u, double rel_tol,
                   int max_iterations, double *rel_residual)
{
  if (!h || !d_fine_rhs || !d_fine_u || max_iterations < 0)
    return SLOD_ERR_ARGUMENT;
  if (problem >= (uint32_t)h->cfg.n_problems)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_fem_solve: problem out of range");
  const int s = h->cfg.spacedim;
  for (int f = 0; f < s; ++f)
    if (!h->coef_set[(size_t)problem * 2 + f])
      return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_fem_solve: coefficient not set");
  if (const int rc = slod_enter(h, nullptr, nullptr))
    return rc;
  const size_t cs = (size_t)problem * h->NE * h->NE * 4;
  return fem_solve_grid(h, "slod_fem_solve", h->NE, h->d_coef[0] + cs, s == 2 ? h->d_coef[1] + cs : nullptr, d_fine_rhs,
                        d_fine_u, rel_tol, max_iterations, rel_residual);
}

// ---- coarse FEM(H) reference problem (LOD.cc:1103-1237) ----
static void launch_coarse_sample(const slod_handle *h, uint32_t problem, int field, double *d_out, hipStream_t st)
{
  const size_t cnt = (size_t)h->N * h->N * 4;
  hipLaunchKernelGGL(k_coarse_sample, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, h->N, h->cfg.n_subdivisions,
                     coarse_sample_rule(h->cfg.n_subdivisions), h->d_coef[field] + (size_t)problem * h->NE * h->NE * 4, d_out);
}

int slod_coarse_coefficient(slod_handle *h, uint32_t problem, int field, double *d_out, void *hip_stream)
{
  if (!h || !d_out)
    return SLOD_ERR_ARGUMENT;
  if (problem >= (uint32_t)h->cfg.n_problems || field < 0 || field >= h->cfg.spacedim)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_coarse_coefficient: problem/field out of range");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  if (!h->coef_set[(size_t)problem * 2 + field])
    return slod_fail(h, SLOD_ERR_STATE, "slod_coarse_coefficient: coefficient not set");
  launch_coarse_sample(h, problem, field, d_out, st);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_coarse_coefficient");
}

int slod_coarse_fem_rhs(slod_handle *h, const double *d_f_cqp, double *d_coarse_rhs, void *hip_stream)
{
  if (!h || !d_coarse_rhs)
    return SLOD_ERR_ARGUMENT;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int    nn = (h->N + 1) * (h->N + 1);
  const double H  = 1.0 / h->N;
  // k_fem_rhs with NE := N, h := H: FE_Q_iso_Q1(1) with QIterated(QGauss(2), 1) (coarse_fem_subdivisions = 1)
  hipLaunchKernelGGL(k_fem_rhs, dim3((nn + 255) / 256), dim3(256), 0, st, h->N, h->cfg.spacedim, H * H * 0.25, d_f_cqp,
                     d_coarse_rhs);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_coarse_fem_rhs");
}

int slod_coarse_fem_solve(slod_handle *h, uint32_t problem, const double *d_coarse_rhs, double *d_coarse_u, double rel_tol,
                          int max_iterations, double *rel_residual)
{
  if (!h || !d_coarse_rhs || !d_coarse_u || max_iterations < 0)
    return SLOD_ERR_ARGUMENT;
  if (problem >= (uint32_t)h->cfg.n_problems)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_coarse_fem_solve: problem out of range");
  if (const int rc = slod_enter(h, nullptr, nullptr))
    return rc;
  const int s = h->cfg.spacedim;
  for (int f = 0; f < s; ++f)
    if (!h->coef_set[(size_t)problem * 2 + f])
      return slod_fail(h, SLOD_ERR_STATE, "slod_coarse_fem_solve: coefficient not set");
  const size_t       cnt = (size_t)h->N * h->N * 4;
  SlodDevBuf<double> d_cc; // the coefficient at the coarse Gauss points, one field after the other
  hipError_t         e = d_cc.alloc((size_t)s * cnt);
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_coarse_fem_solve: sampled coefficient");
  for (int f = 0; f < s && e == hipSuccess; ++f)
    {
      launch_coarse_sample(h, problem, f, d_cc.get() + (size_t)f * cnt, h->stream);
      e = hipGetLastError();
    }
  // fem_solve_grid synchronises the handle's stream before it returns: d_cc is idle when it is freed
  const int rc = e == hipSuccess ? fem_solve_grid(h, "slod_coarse_fem_solve", h->N, d_cc.get(), s == 2 ? d_cc.get() + cnt : nullptr,
                                                  d_coarse_rhs, d_coarse_u, rel_tol, max_iterations, rel_residual)
                                 : slod_hip_fail(h, e, "slod_coarse_fem_solve: k_coarse_sample");
  if (rc < 0)
    (void)hipStreamSynchronize(h->stream);
  return rc;
}

int slod_coarse_interpolate(slod_handle *h, const double *d_coarse, double *d_fine, void *hip_stream)
{
  if (!h || !d_coarse || !d_fine)
    return SLOD_ERR_ARGUMENT;
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const int np = h->NE + 1;
  // up to 8 node rows per block on large grids (with one store per thread the kernel is bound by workgroup
  // dispatch), but never fewer than 256 blocks per column of blocks: small grids need every CU
  const int rows = std::min({np, std::max((np + 7) / 8, 256), 65535});
  hipLaunchKernelGGL(k_coarse_prolong, dim3((unsigned)((np + 255) / 256), (unsigned)rows), dim3(256), 0, st, h->N,
                     h->cfg.n_subdivisions, h->cfg.spacedim, d_coarse, d_fine);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_coarse_interpolate");
}

} // extern "C"
#pragma GCC visibility pop
