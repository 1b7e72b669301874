// The eigenvalue problem on the LOD space (the reference has no counterpart: it solves one stationary problem,
// LOD.cc:976-1002):
//   slod_lod_matrix_symmetrize  out = (A + A^T) / 2 on the block rows, bit-symmetric
//   slod_lod_eigs               the lowest eigenpairs of  A u = lambda M u  by block inverse iteration with Rayleigh-Ritz
// An outer iteration is  Y = M X,  A Z = Y (the multi-column CG of slod_lod_multi.hip),  W = A Z,  V = M Z
// (k_lod_apply of slod_lod_time.hip) and three kernels of this file on the tall-skinny block [Z | W | V] (nrow x m,
// m <= 64 columns):
//   k_eig_gram / k_eig_gram_sum  Ga = sym(Z^T W), Gm = sym(Z^T V): one pass over the rows, slab partials, ordered sum
//   k_eig_ritz                   Ga Q = Gm Q Theta, Q^T Gm Q = I in one workgroup out of LDS
//   k_eig_rotate                 X = Z Q; AX = W Q and MX = V Q stay in registers for the residual partials
// Every reduction has a fixed order (no atomics): the same inputs give the same bits.
//   slod_lod_eigs_direct / slod_lod_eigs_ensemble_direct   the same outer iteration with  S Z = Y  on a banded Cholesky
//                                factor of S = A - sigma M (slod_lod_factor.hip) in place of the CG, for one pencil or for
//                                the K pencils of a coefficient ensemble
// The kernels of this file carry the member on blockIdx.y: member k works on columns k m .. k m + m - 1 of the block
// vectors and on its own partials, G, Q, theta, residuals, status and done word.  A single pencil is the ensemble of one
// member.  k_eig_apply is the product of a member's matrix with its m columns.
// The CG path and the paths on a factor share the workspace layout (EigSpace), the start block (eig_start_launch), the
// five launches of the Rayleigh-Ritz pass (eig_ritz_pass), the common argument checks (eig_check) and the text of
// SLOD_ERR_NUMERIC (eig_rank_message); product, inner solve, stop rule and read-back are each path's own.
#include "slod_lod_system.hip.h"
#include "slod_lod_tile.hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace
{
  constexpr int    EG_COLS = LOD_COLS; // block columns: one column chunk (slod_lod_tile.hip.h), and what fits the Ritz LDS
  constexpr double EG_EPS  = 2.220446049250313e-16;

  // out = (A + A^T) / 2 per word (lod_symmetrize_word, slod_lod_system.hip.h)
  __global__ __launch_bounds__(256) void k_lod_symmetrize(int NP, int s, int cap, const double *__restrict__ values,
                                                         const uint32_t *__restrict__ cols, double *__restrict__ out)
  {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w < (size_t)NP * cap * s * s)
      out[w] = lod_symmetrize_word(NP, s, cap, values, 1, cols, w);
  }

  // ---------------------------------------------------------------------------------
  // Start block: column j = (mode t = j / s, component d = j % s) is the discrete sine mode (a_t, b_t) on the centre
  // cells of the patches, in component d.
  // ---------------------------------------------------------------------------------
  struct EigModes
  {
    unsigned char a[EG_COLS], b[EG_COLS];
  };

  __global__ __launch_bounds__(256) void k_eig_start(const SlodGrid G, int NP, int s, int m, const EigModes md, double *x, size_t ld_x)
  {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (size_t)NP * s * m)
      return;
    x += (size_t)blockIdx.y * m; // the member's columns
    const size_t i = w / m;
    const int    j = (int)(w - i * m), e = (int)(i % s), t = j / s, d = j - t * s;
    int          cx, cy;
    grid_centre(G, (uint32_t)(i / s), cx, cy);
    const double sx = sin(md.a[t] * M_PI * (cx + 0.5) / G.N), sy = sin(md.b[t] * M_PI * (cy + 0.5) / G.N);
    x[i * ld_x + j] = d == e ? sx * sy : 0.0;
  }

  // The start block of slod_lod_eigs_shift_direct: entry (caller's row i, column j) is the hash of include/slod.h, a
  // splitmix64 step on (i << 32 | j) mapped to [-1, 1); the same block for every member (blockIdx.y)
  __global__ __launch_bounds__(256) void k_eig_start_hash(int nrow, int m, double *x, size_t ld_x)
  {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (size_t)nrow * m)
      return;
    x += (size_t)blockIdx.y * m;
    const size_t       i = w / m, j = w - i * m;
    unsigned long long z = ((unsigned long long)i << 32 | (unsigned long long)j) + 0x9E3779B97F4A7C15ull;
    z                    = (z ^ z >> 30) * 0xBF58476D1CE4E5B9ull;
    z                    = (z ^ z >> 27) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    x[i * ld_x + j] = (double)(z >> 11) * 0x1p-52 - 1.0;
  }

  // ---------------------------------------------------------------------------------
  // Gram products.  A block takes slabs of GR_ROWS rows (slab g = blockIdx.x, += gridDim.x, as k_lod_apply walks its
  // groups), stages the rows of Z, W, V in LDS (48 KiB) and accumulates Z^T W and Z^T V: thread (ti, tj) of the
  // 16 x 16 grid holds the 4 x 4 tile (4 ti.., 4 tj..) of both products, one fma chain per entry over the rows of
  // the slab in ascending order.  One partial pair per slab; k_eig_gram_sum adds the slabs in ascending order.
  // ---------------------------------------------------------------------------------
  constexpr int GR_ROWS = 32, GR_BLOCK = 256, GR_MAX_BLOCKS = 512;

  __global__ __launch_bounds__(GR_BLOCK) void k_eig_gram(int nrow, int m, int nslab, const double *__restrict__ Z,
                                                        const double *__restrict__ W, const double *__restrict__ V, size_t ld,
                                                        double *__restrict__ partial)
  {
    __shared__ double sz[GR_ROWS][EG_COLS], sw[GR_ROWS][EG_COLS], sv[GR_ROWS][EG_COLS];
    Z += (size_t)blockIdx.y * m, W += (size_t)blockIdx.y * m, V += (size_t)blockIdx.y * m;
    partial += (size_t)blockIdx.y * nslab * 2 * m * m;
    const int i0 = 4 * (threadIdx.x >> 4), j0 = 4 * (threadIdx.x & 15), m4 = (m + 3) & ~3;
    for (int g = blockIdx.x; g < nslab; g += gridDim.x)
      {
        const int r0 = g * GR_ROWS, nr = min(GR_ROWS, nrow - r0);
        for (int idx = threadIdx.x; idx < GR_ROWS * m4; idx += GR_BLOCK)
          {
            const int    lr = idx / m4, c = idx - lr * m4;
            const bool   in = lr < nr && c < m; // the columns m .. m4 pad the last tile with zeros
            const size_t at = (size_t)(r0 + lr) * ld + c;
            sz[lr][c]       = in ? Z[at] : 0.0;
            sw[lr][c]       = in ? W[at] : 0.0;
            sv[lr][c]       = in ? V[at] : 0.0;
          }
        __syncthreads();
        if (i0 < m && j0 < m)
          {
            double ga[4][4], gm[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b)
                ga[a][b] = gm[a][b] = 0.0;
            for (int r = 0; r < nr; ++r)
              {
                double z[4], w[4], v[4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
                  {
                    z[a] = sz[r][i0 + a];
                    w[a] = sw[r][j0 + a];
                    v[a] = sv[r][j0 + a];
                  }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                  for (int b = 0; b < 4; ++b)
                    {
                      ga[a][b] = fma(z[a], w[b], ga[a][b]);
                      gm[a][b] = fma(z[a], v[b], gm[a][b]);
                    }
              }
            double *pa = partial + (size_t)g * 2 * m * m, *pm = pa + (size_t)m * m;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b)
                if (i0 + a < m && j0 + b < m)
                  {
                    pa[(i0 + a) * m + j0 + b] = ga[a][b];
                    pm[(i0 + a) * m + j0 + b] = gm[a][b];
                  }
          }
        __syncthreads();
      }
  }

  // G[which][i][j] = (S_ij + S_ji) / 2, S = the sum of the slab partials in ascending slab order
  __global__ __launch_bounds__(256) void k_eig_gram_sum(int m, int nslab, const double *__restrict__ partial, double *__restrict__ G)
  {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x, mm = m * m;
    if (idx >= 2 * mm)
      return;
    partial += (size_t)blockIdx.y * nslab * 2 * mm, G += (size_t)blockIdx.y * 2 * mm;
    const int which = idx / mm, ij = idx - which * mm, i = ij / m, j = ij - i * m;
    double    a = 0.0, b = 0.0;
    for (int g = 0; g < nslab; ++g)
      {
        const double *P = partial + ((size_t)g * 2 + which) * mm;
        a += P[i * m + j];
        b += P[j * m + i];
      }
    G[idx] = 0.5 * (a + b);
  }

  // ---------------------------------------------------------------------------------
  // The Ritz problem  Ga Q = Gm Q Theta,  Q^T Gm Q = I,  Theta ascending, in one workgroup: three m x m matrices in
  // LDS (row pitch 65 doubles, 97.5 KiB of the 160 KiB).
  //   Gm = L L^T             right-looking Cholesky; a pivot that is not above 4 m eps times the diagonal entry it
  //                          started from is taken as non-positive: *status = column + 1, nothing else is written
  //   C = L^-1 Ga L^-T       two triangular solves, a thread per column, then per row; symmetrised
  //   C U = U D              cyclic Jacobi, the pairs of a sweep in round-robin order (m - 1 rounds of m / 2 disjoint
  //                          pairs: the rotations of a round commute, so the order is fixed and the result does not
  //                          depend on the thread that applies a rotation), until off(C) <= m eps ||C||_F at the head
  //                          of a sweep or RZ_SWEEPS sweeps
  //   sort D ascending, ties by index;  Q = L^-T U (sorted columns).  near != 0 (slod_lod_eigs_shift_direct): the key is
  //   |D_j - sigma| ascending, ties by ascending D_j, then by index; with near = 0 the two keys agree and the order, hence
  //   every word, is that of the ascending sort
  // ---------------------------------------------------------------------------------
  constexpr int RZ_LD = EG_COLS + 1, RZ_BLOCK = 256, RZ_SWEEPS = 30;

  __global__ __launch_bounds__(RZ_BLOCK) void k_eig_ritz(int m, const double *__restrict__ G, double *__restrict__ Q,
                                                        double *__restrict__ theta, int *__restrict__ status,
                                                        const int *__restrict__ done, int near, double sigma)
  {
    __shared__ double A[EG_COLS * RZ_LD], L[EG_COLS * RZ_LD], U[EG_COLS * RZ_LD];
    __shared__ double s_c[EG_COLS / 2], s_s[EG_COLS / 2], s_d[EG_COLS], s_off[EG_COLS], s_fro[EG_COLS];
    __shared__ int    s_p[EG_COLS / 2], s_q[EG_COLS / 2], s_perm[EG_COLS], s_stop;
    const int tid = threadIdx.x, mm = m * m;
    if (done[blockIdx.y]) // a member that has stopped keeps its last Q and theta
      return;
    G += (size_t)blockIdx.y * 2 * mm, Q += (size_t)blockIdx.y * mm, theta += (size_t)blockIdx.y * m, status += blockIdx.y;
    for (int idx = tid; idx < mm; idx += RZ_BLOCK)
      {
        const int i = idx / m, j = idx - i * m;
        A[i * RZ_LD + j] = G[idx];
        L[i * RZ_LD + j] = G[mm + idx];
        U[i * RZ_LD + j] = i == j ? 1.0 : 0.0;
      }
    __syncthreads();
    // ---- Cholesky, lower triangle of L in place
    for (int k = 0; k < m; ++k)
      {
        if (tid == 0)
          {
            const double piv = L[k * RZ_LD + k], orig = G[mm + k * m + k];
            const bool   ok = piv > 0.0 && piv > (4 * m * EG_EPS) * orig;
            // (one store per branch: with `s_stop = ok ? 0 : k + 1` ahead of the branch, hipcc of ROCm 7 selected the value on
            // SCC, which the vector compare of the threshold does not set, and a positive pivot below the threshold went on)
            if (ok)
              {
                L[k * RZ_LD + k] = sqrt(piv);
                s_stop           = 0;
              }
            else
              s_stop = k + 1;
          }
        __syncthreads();
        if (s_stop)
          {
            if (tid == 0)
              *status = s_stop;
            return;
          }
        const double d = L[k * RZ_LD + k];
        for (int i = k + 1 + tid; i < m; i += RZ_BLOCK)
          L[i * RZ_LD + k] /= d;
        __syncthreads();
        const int n = m - k - 1;
        for (int idx = tid; idx < n * n; idx += RZ_BLOCK)
          {
            const int i = k + 1 + idx / n, j = k + 1 + idx % n;
            if (j <= i)
              L[i * RZ_LD + j] = fma(-L[i * RZ_LD + k], L[j * RZ_LD + k], L[i * RZ_LD + j]);
          }
        __syncthreads();
      }
    // ---- A <- L^-1 A (thread = column), A <- A L^-T (thread = row), symmetrise
    if (tid < m)
      for (int i = 0; i < m; ++i)
        {
          double acc = A[i * RZ_LD + tid];
          for (int k = 0; k < i; ++k)
            acc = fma(-L[i * RZ_LD + k], A[k * RZ_LD + tid], acc);
          A[i * RZ_LD + tid] = acc / L[i * RZ_LD + i];
        }
    __syncthreads();
    if (tid < m)
      for (int j = 0; j < m; ++j)
        {
          double acc = A[tid * RZ_LD + j];
          for (int k = 0; k < j; ++k)
            acc = fma(-A[tid * RZ_LD + k], L[j * RZ_LD + k], acc);
          A[tid * RZ_LD + j] = acc / L[j * RZ_LD + j];
        }
    __syncthreads();
    for (int idx = tid; idx < mm; idx += RZ_BLOCK)
      {
        const int i = idx / m, j = idx - i * m;
        if (j < i)
          {
            const double v   = 0.5 * (A[i * RZ_LD + j] + A[j * RZ_LD + i]);
            A[i * RZ_LD + j] = v;
            A[j * RZ_LD + i] = v;
          }
      }
    __syncthreads();
    // ---- cyclic Jacobi
    const int n2 = (m + 1) & ~1, nround = n2 - 1, npair = n2 / 2;
    for (int sweep = 0; sweep < RZ_SWEEPS; ++sweep)
      {
        if (tid < m)
          {
            double off = 0.0, fro = 0.0;
            for (int j = 0; j < m; ++j)
              {
                const double v = A[tid * RZ_LD + j];
                fro            = fma(v, v, fro);
                off            = j == tid ? off : fma(v, v, off);
              }
            s_off[tid] = off;
            s_fro[tid] = fro;
          }
        __syncthreads();
        if (tid == 0)
          {
            double off = 0.0, fro = 0.0;
            for (int i = 0; i < m; ++i)
              {
                off += s_off[i];
                fro += s_fro[i];
              }
            const double tol = m * EG_EPS;
            s_stop           = off <= tol * tol * fro ? 1 : 0;
          }
        __syncthreads();
        if (s_stop)
          break;
        for (int r = 0; r < nround; ++r)
          {
            if (tid < npair)
              {
                // circle method: n2 - 1 stays, the others turn
                const int a = tid == 0 ? n2 - 1 : (r + tid) % nround, b = tid == 0 ? r : (r - tid + nround) % nround;
                const int p = min(a, b), q = max(a, b);
                double    c = 1.0, s = 0.0;
                if (q < m)
                  {
                    const double apq = A[p * RZ_LD + q];
                    if (apq != 0.0)
                      {
                        const double tau = (A[q * RZ_LD + q] - A[p * RZ_LD + p]) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                      }
                  }
                s_p[tid] = q < m && s != 0.0 ? p : -1; // the padding index of an odd m, or nothing to rotate
                s_q[tid] = q;
                s_c[tid] = c;
                s_s[tid] = s;
              }
            __syncthreads();
            // columns p, q of A and of U
            for (int idx = tid; idx < npair * m; idx += RZ_BLOCK)
              {
                const int k = idx / m, i = idx - k * m, p = s_p[k], q = s_q[k];
                if (p < 0)
                  continue;
                const double c = s_c[k], s = s_s[k];
                double       x = A[i * RZ_LD + p], y = A[i * RZ_LD + q];
                A[i * RZ_LD + p] = c * x - s * y;
                A[i * RZ_LD + q] = s * x + c * y;
                x = U[i * RZ_LD + p], y = U[i * RZ_LD + q];
                U[i * RZ_LD + p] = c * x - s * y;
                U[i * RZ_LD + q] = s * x + c * y;
              }
            __syncthreads();
            // rows p, q of A
            for (int idx = tid; idx < npair * m; idx += RZ_BLOCK)
              {
                const int k = idx / m, j = idx - k * m, p = s_p[k], q = s_q[k];
                if (p < 0)
                  continue;
                const double c = s_c[k], s = s_s[k];
                const double x = A[p * RZ_LD + j], y = A[q * RZ_LD + j];
                A[p * RZ_LD + j] = c * x - s * y;
                A[q * RZ_LD + j] = s * x + c * y;
              }
            __syncthreads();
          }
      }
    // ---- sort, Q = L^-T U
    if (tid < m)
      s_d[tid] = A[tid * RZ_LD + tid];
    __syncthreads();
    if (tid < m)
      {
        const double v = s_d[tid], key = near ? fabs(v - sigma) : v;
        int          rank = 0;
        for (int k = 0; k < m; ++k)
          {
            const double dk = s_d[k], kk = near ? fabs(dk - sigma) : dk;
            rank += (kk < key || (kk == key && (dk < v || (dk == v && k < tid)))) ? 1 : 0;
          }
        s_perm[rank] = tid;
      }
    __syncthreads();
    if (tid < m)
      {
        const int src = s_perm[tid];
        for (int i = m - 1; i >= 0; --i)
          {
            double acc = U[i * RZ_LD + src];
            for (int k = i + 1; k < m; ++k)
              acc = fma(-L[k * RZ_LD + i], A[k * RZ_LD + tid], acc);
            A[i * RZ_LD + tid] = acc / L[i * RZ_LD + i];
          }
        theta[tid] = s_d[src];
      }
    __syncthreads();
    for (int idx = tid; idx < mm; idx += RZ_BLOCK)
      Q[idx] = A[(idx / m) * RZ_LD + idx % m];
    if (tid == 0)
      *status = 0;
  }

  // ---------------------------------------------------------------------------------
  // [X | AX | MX] = [Z | W | V] Q: Q and a slab of RT_ROWS rows in LDS (72 KiB with the residual buffers), an item is
  // one (row, column) with its three fma chains over k ascending.  X goes to d_x; AX and MX are consumed at once:
  // (AX - theta MX)^2 and MX^2, summed over the rows of the slab in ascending order into one partial per
  // (slab, column); k_eig_residual adds the slabs in ascending order.  Nothing is written after a failed Ritz step.
  // ---------------------------------------------------------------------------------
  constexpr int RT_ROWS = LOD_ROWS, RT_BLOCK = LOD_BLOCK, RT_MAX_BLOCKS = 1024; // a slab is a reduction group

  __global__ __launch_bounds__(RT_BLOCK) void k_eig_rotate(int nrow, int m, int nslab, const double *__restrict__ Z,
                                                          const double *__restrict__ W, const double *__restrict__ V,
                                                          const double *__restrict__ Q, const double *__restrict__ theta,
                                                          const int *__restrict__ status, const int *__restrict__ done, size_t ld,
                                                          double *__restrict__ x, size_t ld_x, double *__restrict__ p_rr,
                                                          double *__restrict__ p_mm)
  {
    __shared__ double sq[EG_COLS][EG_COLS];
    __shared__ double sz[RT_ROWS][EG_COLS], sw[RT_ROWS][EG_COLS], sv[RT_ROWS][EG_COLS];
    __shared__ double b_rr[RT_ROWS][EG_COLS], b_mm[RT_ROWS][EG_COLS];
    if (done[blockIdx.y] || status[blockIdx.y] != 0)
      return;
    Z += (size_t)blockIdx.y * m, W += (size_t)blockIdx.y * m, V += (size_t)blockIdx.y * m, x += (size_t)blockIdx.y * m;
    Q += (size_t)blockIdx.y * m * m, theta += (size_t)blockIdx.y * m;
    p_rr += (size_t)blockIdx.y * nslab * m, p_mm += (size_t)blockIdx.y * nslab * m;
    for (int idx = threadIdx.x; idx < m * m; idx += RT_BLOCK)
      sq[idx / m][idx % m] = Q[idx];
    for (int g = blockIdx.x; g < nslab; g += gridDim.x)
      {
        for (int idx = threadIdx.x; idx < RT_ROWS * m; idx += RT_BLOCK)
          {
            const int    lr = idx / m, c = idx - lr * m, i = g * RT_ROWS + lr;
            const size_t at = (size_t)i * ld + c;
            sz[lr][c]       = i < nrow ? Z[at] : 0.0;
            sw[lr][c]       = i < nrow ? W[at] : 0.0;
            sv[lr][c]       = i < nrow ? V[at] : 0.0;
          }
        __syncthreads();
        for (int idx = threadIdx.x; idx < RT_ROWS * m; idx += RT_BLOCK)
          {
            const int lr = idx / m, j = idx - lr * m, i = g * RT_ROWS + lr;
            double    xv = 0.0, ax = 0.0, mx = 0.0;
            for (int k = 0; k < m; ++k)
              {
                const double q = sq[k][j];
                xv             = fma(sz[lr][k], q, xv);
                ax             = fma(sw[lr][k], q, ax);
                mx             = fma(sv[lr][k], q, mx);
              }
            double rr = 0.0, mm = 0.0;
            if (i < nrow)
              {
                x[(size_t)i * ld_x + j] = xv;
                const double r          = fma(-theta[j], mx, ax);
                rr                      = r * r;
                mm                      = mx * mx;
              }
            b_rr[lr][j] = rr;
            b_mm[lr][j] = mm;
          }
        __syncthreads();
        if ((int)threadIdx.x < m)
          {
            p_rr[(size_t)g * m + threadIdx.x] = slod_lod_group_sum(b_rr, threadIdx.x);
            p_mm[(size_t)g * m + threadIdx.x] = slod_lod_group_sum(b_mm, threadIdx.x);
          }
        __syncthreads();
      }
  }

  // res_j = ||AX_j - theta_j MX_j|| / (|theta_j| ||MX_j||), one thread per column.  The member stops (done = 1: its Ritz,
  // rotate and residual kernels return at entry from then on) when res_j <= tol for all j < n_eig, or when its Ritz step
  // failed; its X, theta and residuals stay those of this iteration.
  __global__ __launch_bounds__(EG_COLS) void k_eig_residual(int m, int n_eig, int nslab, double tol, const double *__restrict__ p_rr,
                                                          const double *__restrict__ p_mm, const double *__restrict__ theta,
                                                          const int *__restrict__ status, double *__restrict__ res,
                                                          int *__restrict__ done)
  {
    __shared__ int s_open;
    const int      j = threadIdx.x, k = blockIdx.y;
    if (done[k])
      return;
    if (status[k] != 0)
      {
        if (j == 0)
          done[k] = 1;
        return;
      }
    p_rr += (size_t)k * nslab * m, p_mm += (size_t)k * nslab * m, theta += (size_t)k * m, res += (size_t)k * m;
    if (j == 0)
      s_open = 0;
    __syncthreads();
    if (j < m)
      {
        const double rr = slod_lod_ordered_sum(p_rr, nslab, m, j), mm = slod_lod_ordered_sum(p_mm, nslab, m, j);
        const double r  = sqrt(rr) / (fabs(theta[j]) * sqrt(mm));
        res[j]          = r;
        if (j < n_eig && !(r <= tol))
          s_open = 1;
      }
    __syncthreads();
    if (j == 0 && !s_open)
      done[k] = 1;
  }

  // ---------------------------------------------------------------------------------
  // Y_k = A_k X_k for the m columns of member k = blockIdx.y: the tiling of k_lod_apply (slod_lod_time.hip) with the m
  // columns on lanes, and its fma chain (slod_lod_row_product<false>, slod_lod_tile.hip.h: slots ascending, an unused slot
  // reads the row's own patch and adds nothing, no branch) on the words of member k of an ensemble matrix, ld_m apart:
  // the lanes of a row share one word, and a column has the bits slod_lod_apply_multi gives on the de-interleaved matrix.
  // ---------------------------------------------------------------------------------
  constexpr int AP_MAX_BLOCKS = 1024; // blocks per member, as k_lod_apply per chunk

  __global__ __launch_bounds__(LOD_BLOCK) void k_eig_apply(int nrow, int s, int cap, int NP, int m, int ngroup,
                                                         const double *__restrict__ values, size_t ld_m,
                                                         const uint32_t *__restrict__ cols, const double *__restrict__ x, size_t ld_x,
                                                         double *__restrict__ y, size_t ld_y)
  {
    values += blockIdx.y, x += (size_t)blockIdx.y * m, y += (size_t)blockIdx.y * m;
    for (int g = blockIdx.x; g < ngroup; g += gridDim.x)
      for (int idx = threadIdx.x; idx < LOD_ROWS * m; idx += LOD_BLOCK)
        {
          const int lr = idx / m, col = idx - lr * m, i = g * LOD_ROWS + lr;
          if (i >= nrow)
            continue;
          const int    p = i / s, d = i - p * s;
          const size_t slot0 = (size_t)p * cap;
          double       acc = 0.0;
          for (int j = 0; j < cap; ++j)
            {
              const uint32_t q = cols[slot0 + j];
              const bool     used = q < (uint32_t)NP;
              const size_t   qs = (size_t)(used ? q : (uint32_t)p) * s;
              const double  *a = values + ((slot0 + j) * s * s + d * s) * ld_m;
              for (int e = 0; e < s; ++e)
                {
                  const double t = fma(a[e * ld_m], x[(qs + e) * ld_x + col], acc);
                  acc            = used ? t : acc;
                }
            }
          y[(size_t)i * ld_y + col] = acc;
        }
  }

  // the modes of the start block of m columns: the pairs (a, b) of {1..N}^2 in ascending a^2 + b^2, ties by ascending a
  EigModes eig_sine_modes(const slod_handle *h, int m)
  {
    const int                        s = h->cfg.spacedim, side = std::min(h->N, EG_COLS), n_modes = (m + s - 1) / s;
    std::vector<std::pair<int, int>> ab;
    for (int a = 1; a <= side; ++a)
      for (int b = 1; b <= side; ++b)
        ab.emplace_back(a, b);
    std::sort(ab.begin(), ab.end(), [](const std::pair<int, int> &u, const std::pair<int, int> &v) {
      const int nu = u.first * u.first + u.second * u.second, nv = v.first * v.first + v.second * v.second;
      return nu != nv ? nu < nv : u.first < v.first;
    });
    EigModes md{};
    for (int t = 0; t < n_modes; ++t)
      {
        md.a[t] = (unsigned char)ab[t].first;
        md.b[t] = (unsigned char)ab[t].second;
      }
    return md;
  }

  // ---------------------------------------------------------------------------------
  // What the CG path (slod_lod_eigs) and the paths on a factor (eigs_direct) share.  Each keeps its own product
  // (k_lod_apply or k_eig_apply), its own stop rule (the host's test of the residuals, or the done words of the device)
  // and its own read-back.
  // ---------------------------------------------------------------------------------
  // The checks both paths make, in their order.  inner: the CG path, which looks at ld_x right behind n_block and names
  // the tolerance and the limit of its inner solve along with the outer ones.
  int eig_check(const slod_handle *h, const std::string &who, int n_eig, int n_block, int start, double tol, int max_outer,
                bool inner = false, size_t ld_x = 0, double inner_rel_tol = 1.0, int inner_max_iterations = 0)
  {
    if (n_eig < 1 || n_block < n_eig)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_eig < 1 or n_block < n_eig");
    if (n_block > EG_COLS || n_block > h->NP * h->cfg.spacedim)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": n_block above 64 or above the number of rows");
    if (inner)
      if (const int rc = slod_check_ld(h, who.c_str(), "n_block", n_block, {ld_x}))
        return rc;
    if (start != 0 && start != 1)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + ": start is neither 0 nor 1");
    if (!(tol > 0.0) || !(inner_rel_tol > 0.0))
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (inner ? ": tol or inner_rel_tol is not positive" : ": tol is not positive"));
    if (max_outer < 1 || inner_max_iterations < 0)
      return slod_fail(h, SLOD_ERR_ARGUMENT, who + (inner ? ": max_outer < 1 or inner_max_iterations < 0" : ": max_outer < 1"));
    return SLOD_OK;
  }

  // The device arrays of the outer iteration for K members of m columns each (one pencil: K = 1): Y, Z, W, V of K m
  // columns, per member the slab partials, Ga | Gm and Q, then theta | residuals | status | done of all members
  // (consecutive: the host reads them in one copy; the ints of the members in whole doubles)
  struct EigSpace
  {
    int     nrow, m, K, n_gslab, n_rslab; // n_rslab: the groups of lod_shape are the slabs of k_eig_rotate and k_eig_apply
    size_t  ldw, nint;
    double *Y, *Z, *W, *V, *partial, *G, *Q, *p_rr, *p_mm, *theta, *res;
    int    *status, *d_done;
    EigSpace(const LodShape &w, int m, int K)
      : nrow(w.nrow), m(m), K(K), n_gslab((w.nrow + GR_ROWS - 1) / GR_ROWS), n_rslab(w.ngroup), ldw((size_t)K * m), nint(((size_t)K + 1) / 2)
    {}
    void carve(SlodCarver &c)
    {
      const size_t nvec = (size_t)nrow * ldw, mm = (size_t)m * m;
      Y = c.take(nvec), Z = c.take(nvec), W = c.take(nvec), V = c.take(nvec);
      partial = c.take(K * 2 * mm * n_gslab), G = c.take(K * 2 * mm), Q = c.take(K * mm);
      p_rr = c.take(ldw * n_rslab), p_mm = c.take(ldw * n_rslab);
      theta = c.take(ldw), res = c.take(ldw), status = (int *)c.take(nint), d_done = (int *)c.take(nint);
    }
  };

  // start = 0: the library's start block in the m columns of every member, sine modes or (hashed) the hashed block
  void eig_start_launch(const slod_handle *h, hipStream_t st, bool hashed, int m, int K, double *d_x, size_t ld_x)
  {
    const int  s = h->cfg.spacedim, nrow = h->NP * s;
    const dim3 grid((unsigned)(((size_t)nrow * m + 255) / 256), (unsigned)K);
    if (hashed)
      hipLaunchKernelGGL(k_eig_start_hash, grid, dim3(256), 0, st, nrow, m, d_x, ld_x);
    else
      hipLaunchKernelGGL(k_eig_start, grid, dim3(256), 0, st, slod_grid_of(h), h->NP, s, m, eig_sine_modes(h, m), d_x, ld_x);
  }

  // The Rayleigh-Ritz pass on [Z | W | V], five launches with the member on blockIdx.y: the Gram matrices, the Ritz pairs
  // (near: ordered by their distance from sigma), X = Z Q, and the residuals of the first n_eig pairs against tol.  The
  // slabs of k_eig_rotate are the groups of lod_shape(h, m) and m <= 64 is one column chunk, so its grid is
  // lod_grid(w, RT_MAX_BLOCKS) with the members on y.
  void eig_ritz_pass(hipStream_t st, const EigSpace &E, int n_eig, double tol, bool near, double sigma, double *d_x, size_t ld_x)
  {
    const int      m = E.m;
    const unsigned K = (unsigned)E.K;
    hipLaunchKernelGGL(k_eig_gram, dim3((unsigned)std::min(E.n_gslab, GR_MAX_BLOCKS), K), dim3(GR_BLOCK), 0, st, E.nrow, m, E.n_gslab,
                       E.Z, E.W, E.V, E.ldw, E.partial);
    hipLaunchKernelGGL(k_eig_gram_sum, dim3((unsigned)((2 * (size_t)m * m + 255) / 256), K), dim3(256), 0, st, m, E.n_gslab, E.partial,
                       E.G);
    hipLaunchKernelGGL(k_eig_ritz, dim3(1, K), dim3(RZ_BLOCK), 0, st, m, E.G, E.Q, E.theta, E.status, E.d_done, near ? 1 : 0, sigma);
    hipLaunchKernelGGL(k_eig_rotate, dim3((unsigned)std::min(E.n_rslab, RT_MAX_BLOCKS), K), dim3(RT_BLOCK), 0, st, E.nrow, m, E.n_rslab,
                       E.Z, E.W, E.V, E.Q, E.theta, E.status, E.d_done, E.ldw, d_x, ld_x, E.p_rr, E.p_mm);
    hipLaunchKernelGGL(k_eig_residual, dim3(1, K), dim3(EG_COLS), 0, st, m, n_eig, E.n_rslab, tol, E.p_rr, E.p_mm, E.theta, E.status,
                       E.res, E.d_done);
  }

  // The text of SLOD_ERR_NUMERIC: k_eig_ritz met a non-positive pivot (status = column + 1); member < 0: a single pencil
  std::string eig_rank_message(const std::string &who, int member, int status, int outer)
  {
    return who + ": " + (member >= 0 ? "member " + std::to_string(member) + ": " : std::string()) +
           "non-positive pivot in the Cholesky of Gm = Z^T M Z at column " + std::to_string(status - 1) + " of outer iteration " +
           std::to_string(outer) + " (rank-deficient block)";
  }

  // The body of slod_lod_eigs_ensemble_direct; slod_lod_eigs_direct is the call with n_members = 1 and ld = 1.  Member k
  // works on columns k m .. k m + m - 1 of d_x and of the workspace vectors.  Arguments are checked here, the factor last.
  // near: the body of slod_lod_eigs_shift(_ensemble)_direct: the Ritz pairs are ordered by their distance from sigma and
  // start = 0 writes the hashed block; without it sigma is not used.
  int eigs_direct(slod_handle *h, const char *who, bool ensemble, bool near, double sigma, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_a_m,
                  const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, int n_members, int n_eig, int n_block, int start,
                  double *d_x, size_t ld_x, double tol, int max_outer, double *eigenvalues, double *residuals, int *member_status)
  {
    const std::string name(who);
    if (!h || !d_stiffness || !d_mass || !d_cols || !d_x || !eigenvalues || !residuals)
      return slod_fail(h, SLOD_ERR_ARGUMENT, name + ": NULL handle, matrix, d_cols, d_x, eigenvalues or residuals");
    const int m = n_block, K = n_members;
    if (const int rc = eig_check(h, name, n_eig, n_block, start, tol, max_outer))
      return rc;
    if (K < 1 || K > 65535)
      return slod_fail(h, SLOD_ERR_ARGUMENT, name + ": n_members < 1 or > 65535");
    if (const int rc = slod_check_ld(h, who, "n_members", K, {ld_a_m, ld_m_m}))
      return rc;
    if (ld_x < (size_t)K * m)
      return slod_fail(h, SLOD_ERR_ARGUMENT, name + (ensemble ? ": leading dimension below n_members * n_block" : ": leading dimension below n_block"));
    if (!member_status)
      return slod_fail(h, SLOD_ERR_ARGUMENT, name + ": NULL member_status");
    if (near && !(sigma - sigma == 0.0))
      return slod_fail(h, SLOD_ERR_ARGUMENT, name + ": sigma is NaN or infinite");
    if (const int rc = slod_lod_factor_check(h, who, f_S, K)) // last: it reads the factor
      return rc;
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const LodShape w = lod_shape(h, m);
    EigSpace       E(w, m, K);
    const size_t   ldw = E.ldw, nint = E.nint, nread = 2 * ldw + 2 * nint; // theta | residuals | status | done
    // one allocation for the whole loop
    SlodDevBuf<double> work;
    SlodCarver         count, hand;
    E.carve(count);
    hipError_t e = work.alloc(count.used);
    hand.base    = work.get();
    if (e == hipSuccess)
      {
        E.carve(hand);
        e = hipMemsetAsync(E.theta, 0, nread * sizeof(double), st);
      }
    std::vector<double> host(nread);
    std::vector<int>    ran((size_t)K, 0), failed_column((size_t)K, 0); // outer iterations of a stopped member, 0 = still open
    int                 outer = 0, open = K;
    if (e == hipSuccess)
      {
        if (start == 0)
          {
            eig_start_launch(h, st, near, m, K, d_x, ld_x);
            e = hipGetLastError();
          }
        const dim3 apply_grid((unsigned)std::min(w.ngroup, AP_MAX_BLOCKS), (unsigned)K);
        auto       apply = [&](const double *values, size_t ld_m, const double *x, size_t ldx, double *y) {
          hipLaunchKernelGGL(k_eig_apply, apply_grid, dim3(LOD_BLOCK), 0, st, w.nrow, w.s, w.cap, w.NP, m, w.ngroup, values, ld_m, d_cols,
                             x, ldx, y, ldw);
        };
        while (e == hipSuccess && open > 0 && outer < max_outer)
          {
            apply(d_mass, ld_m_m, d_x, ld_x, E.Y);
            slod_lod_factor_solve_launch(f_S, st, E.Y, ldw, m, E.Z, ldw, 0, K);
            apply(d_stiffness, ld_a_m, E.Z, ldw, E.W);
            apply(d_mass, ld_m_m, E.Z, ldw, E.V);
            eig_ritz_pass(st, E, n_eig, tol, near, sigma, d_x, ld_x);
            e = hipGetLastError();
            if (e == hipSuccess)
              e = hipMemcpyAsync(host.data(), E.theta, nread * sizeof(double), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
              e = hipStreamSynchronize(st);
            if (e != hipSuccess)
              break;
            ++outer;
            const int *h_status = (const int *)(host.data() + 2 * ldw), *h_done = (const int *)(host.data() + 2 * ldw + nint);
            for (int k = 0; k < K; ++k)
              if (ran[(size_t)k] == 0 && h_done[k])
                {
                  ran[(size_t)k]           = outer;
                  failed_column[(size_t)k] = h_status[k];
                  --open;
                }
          }
      }
    const hipError_t es = hipStreamSynchronize(st); // the workspace is freed on return
    if (e == hipSuccess)
      e = es;
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who);
    std::copy(host.begin(), host.begin() + ldw, eigenvalues);
    std::copy(host.begin() + ldw, host.begin() + 2 * ldw, residuals);
    int worst = 0, bad = -1;
    for (int k = K - 1; k >= 0; --k)
      {
        const bool failed = failed_column[(size_t)k] != 0;
        member_status[k]  = failed ? (int)SLOD_ERR_NUMERIC : (ran[(size_t)k] ? ran[(size_t)k] : outer);
        worst             = std::max(worst, member_status[k]);
        if (failed)
          bad = k;
      }
    if (bad >= 0)
      return slod_fail(h, SLOD_ERR_NUMERIC, eig_rank_message(name, ensemble ? bad : -1, failed_column[(size_t)bad], ran[(size_t)bad]));
    return worst;
  }

} // namespace

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_matrix_symmetrize(slod_handle *h, const double *d_values, const uint32_t *d_cols, double *d_out, void *hip_stream)
{
  if (!h || !d_values || !d_cols || !d_out)
    return SLOD_ERR_ARGUMENT;
  if (d_out == d_values)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_matrix_symmetrize: a row reads other rows, the call cannot run in place");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  const LodShape w = lod_shape(h, 1);
  hipLaunchKernelGGL(k_lod_symmetrize, lod_flat_grid((size_t)w.NP * w.cap * w.s * w.s), dim3(256), 0, st, w.NP, w.s, w.cap, d_values, d_cols, d_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_matrix_symmetrize");
}

int slod_lod_eigs(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, int n_eig, int n_block,
                  int start, double *d_x, size_t ld_x, double tol, int max_outer, double inner_rel_tol, int inner_max_iterations,
                  double *eigenvalues, double *residuals, int *inner_iterations)
{
  if (!h || !d_stiffness || !d_mass || !d_cols || !d_x || !eigenvalues || !residuals)
    return SLOD_ERR_ARGUMENT;
  if (const int rc = eig_check(h, "slod_lod_eigs", n_eig, n_block, start, tol, max_outer, true, ld_x, inner_rel_tol, inner_max_iterations))
    return rc;
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  const int   m = n_block;
  EigSpace    E(lod_shape(h, m), m, 1);
  // one allocation for the whole loop: the arrays of the outer iteration, the workspace of the solve
  SlodLodWork work;
  hipError_t  e = work.alloc(m, [&](SlodCarver &c) { E.carve(c), work.take_solve(c, h); });
  if (e == hipSuccess)
    e = hipMemsetAsync(E.status, 0, 2 * sizeof(double), st); // status and done: the host decides when this loop stops
  int outer = 0, failed_column = 0;
  if (e == hipSuccess)
    {
      if (start == 0)
        {
          eig_start_launch(h, st, false, m, 1, d_x, ld_x);
          e = hipGetLastError();
        }
      std::vector<double> host(2 * (size_t)m + 1); // theta | residuals | status: the last slot holds the int
      bool                done = false;
      while (e == hipSuccess && !done && outer < max_outer)
        {
          slod_lod_apply_launch(h, st, d_mass, d_cols, d_x, ld_x, m, E.Y, (size_t)m);
          e = hipGetLastError();
          if (e == hipSuccess)
            e = work.solve(h, d_stiffness, d_cols, E.Y, (size_t)m, E.Z, (size_t)m, inner_rel_tol, inner_max_iterations);
          if (e != hipSuccess)
            break;
          slod_lod_apply_launch(h, st, d_stiffness, d_cols, E.Z, (size_t)m, m, E.W, (size_t)m);
          slod_lod_apply_launch(h, st, d_mass, d_cols, E.Z, (size_t)m, m, E.V, (size_t)m);
          eig_ritz_pass(st, E, n_eig, tol, false, 0.0, d_x, ld_x);
          e = hipGetLastError();
          if (e == hipSuccess)
            e = hipMemcpyAsync(host.data(), E.theta, host.size() * sizeof(double), hipMemcpyDeviceToHost, st);
          if (e == hipSuccess)
            e = hipStreamSynchronize(st);
          if (e != hipSuccess)
            break;
          if (inner_iterations)
            inner_iterations[outer] = work.last;
          ++outer;
          std::memcpy(&failed_column, &host[2 * (size_t)m], sizeof(int));
          if (failed_column != 0)
            break;
          std::copy(host.begin(), host.begin() + m, eigenvalues);
          std::copy(host.begin() + m, host.begin() + 2 * m, residuals);
          done = true;
          for (int j = 0; j < n_eig; ++j)
            done = done && residuals[j] <= tol;
        }
      // every completed pass ends on a synchronised stream; a failed one waits here: the workspace is freed on return and a
      // queued kernel may still touch it
      if (e != hipSuccess)
        (void)hipStreamSynchronize(st);
    }
  if (e != hipSuccess)
    return slod_hip_fail(h, e, "slod_lod_eigs");
  if (failed_column != 0)
    return slod_fail(h, SLOD_ERR_NUMERIC, eig_rank_message("slod_lod_eigs", -1, failed_column, outer));
  return outer;
}

int slod_lod_eigs_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                         int n_eig, int n_block, int start, double *d_x, size_t ld_x, double tol, int max_outer, double *eigenvalues,
                         double *residuals)
{
  int ran = 0;
  return eigs_direct(h, "slod_lod_eigs_direct", false, false, 0.0, f_S, d_stiffness, 1, d_mass, 1, d_cols, 1, n_eig, n_block, start, d_x, ld_x, tol,
                     max_outer, eigenvalues, residuals, &ran);
}

int slod_lod_eigs_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_a_m, const double *d_mass,
                                  size_t ld_m_m, const uint32_t *d_cols, int n_members, int n_eig, int n_block, int start, double *d_x,
                                  size_t ld_x, double tol, int max_outer, double *eigenvalues, double *residuals, int *member_status)
{
  return eigs_direct(h, "slod_lod_eigs_ensemble_direct", true, false, 0.0, f_S, d_stiffness, ld_a_m, d_mass, ld_m_m, d_cols, n_members, n_eig,
                     n_block, start, d_x, ld_x, tol, max_outer, eigenvalues, residuals, member_status);
}

int slod_lod_eigs_shift_direct(slod_handle *h, slod_lod_factor *f_S, double sigma, const double *d_stiffness, const double *d_mass,
                               const uint32_t *d_cols, int n_eig, int n_block, int start, double *d_x, size_t ld_x, double tol,
                               int max_outer, double *eigenvalues, double *residuals)
{
  int ran = 0;
  return eigs_direct(h, "slod_lod_eigs_shift_direct", false, true, sigma, f_S, d_stiffness, 1, d_mass, 1, d_cols, 1, n_eig, n_block,
                     start, d_x, ld_x, tol, max_outer, eigenvalues, residuals, &ran);
}

int slod_lod_eigs_shift_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, double sigma, const double *d_stiffness, size_t ld_a_m,
                                        const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, int n_members, int n_eig,
                                        int n_block, int start, double *d_x, size_t ld_x, double tol, int max_outer,
                                        double *eigenvalues, double *residuals, int *member_status)
{
  return eigs_direct(h, "slod_lod_eigs_shift_ensemble_direct", true, true, sigma, f_S, d_stiffness, ld_a_m, d_mass, ld_m_m, d_cols,
                     n_members, n_eig, n_block, start, d_x, ld_x, tol, max_outer, eigenvalues, residuals, member_status);
}

} // extern "C"
#pragma GCC visibility pop
