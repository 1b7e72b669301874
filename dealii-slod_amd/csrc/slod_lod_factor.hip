// Direct solver on the LOD space: banded Cholesky  A = L L^T  of a full set of block rows, factored once and used by
// any number of solves (the reference has no counterpart: it runs CG + SSOR once, LOD.cc:990-998):
//   slod_lod_factor_create   band storage, the left-looking factorisation, pivot range and status
//   slod_lod_factor_solve    U = A^-1 RHS on coarse multi-vectors, asynchronous, no allocation, no read-back
//   slod_lod_factor_create_ensemble / _solve_ensemble  the same for the K matrices of a coefficient ensemble: one
//                            allocation of K copies of the storage below, the same kernels with the member on blockIdx.y
//                            (a single factor is the ensemble of one member)
//   slod_lod_factor_create_ldl(_ensemble) / slod_lod_factor_inertia  a second kind of factor in the same storage,
//                            S = L D L^T without pivoting for a symmetric indefinite S = sym(A) - sigma M, with the signs
//                            of D and the growth || |L| |D| |L^T| ||_inf / ||S||_inf; the solve dispatches on the kind, so
//                            every consumer of a factor takes either
//   slod_lod_factor_create_zldl / slod_lod_factor_solve_complex  a third kind in the same tiles, two planes (real,
//                            imaginary) per array: the complex symmetric S_k = alpha_k A + beta_k B = L D L^T (plain
//                            transpose) of every member k, for the frequency response (slod_lod_harmonic.hip); a complex
//                            tile product is four MFMAs into two accumulators; the real consumers refuse this kind
// Ordering: unknown (p, d) has the index r = (cy N + cx) s + d, (cx, cy) the centre cell of p, so the block stencil of a
// row (slot j = cell offset (j % span, j / span) - span / 2, slod_grid.hip.h) is a band of half width
// b = s (w N + w) + s - 1, w = 2 l + 1.
// Storage: tiles of FB x FB = 16 x 16, nb = ceil(n / 16) block rows, bb = (b + 15) / 16 block sub-diagonals; tile
// (I, I - k), k = 1 .. bb, at band[(I (bb + 1) + k) 256] (k = 0 keeps A_II; L_II has an array of its own), column-major inside (entry (r, c) at [c 16 + r]), so the lanes
// of the A operand of v_mfma_f64_16x16x4_f64 (lane l feeds A[l & 15][l >> 4]) read 16 consecutive doubles.  Rows
// n .. 16 nb - 1 are padding with a unit diagonal: their pivots are 1 and their solution is 0.
// Factorisation: one launch per block column K in stream order, no dependency inside a launch (left-looking).  Block
// K + x of the launch forms  T = A_rK - sum_J L_rJ L_KJ^T  on the matrix pipe and, redundantly, the diagonal tile
// A_KK - sum_J L_KJ L_KJ^T, factors that tile in LDS and solves  L_rK L_KK^T = T  by rows.
// Solve: one block of four waves per chunk of 16 columns walks the block rows forwards (L y = b), then backwards
// (L^T x = y).  The tiles of a block row are dealt to the waves round-robin (tile k to wave (k - 1) & 3), every wave
// accumulates its tiles in ascending k, the four partial tiles are added in wave order: a fixed order of summation, and
// a column of an MFMA result depends on its own input column only, so the bits of a column of U depend on the factor and
// that column of RHS alone.  X lives in the caller's d_u (through the row map), which is L2-resident; there is no LDS
// window and so no size-dependent path.
#include "slod_grid.hip.h"
#include "slod_common.hip.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace
{
  constexpr int FB = 16, FT = FB * FB; // tile edge (one MFMA M / N), doubles per tile

  __device__ __forceinline__ double4_t mfma(double a, double b, double4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

  // factor index of unknown (p, d)
  __device__ __forceinline__ int factor_index(const SlodGrid &G, uint32_t p, int d)
  {
    int cx, cy;
    grid_centre(G, p, cx, cy);
    return (cy * G.N + cx) * G.spacedim + d;
  }

  // rowmap[r] = p s + d, the caller's row of factor index r (-1: padding), and the unit diagonal of the padding
  // of every member (blockIdx.y, copies mstride doubles apart)
  __global__ __launch_bounds__(256) void k_factor_rowmap(const SlodGrid G, int n, int npad, int bb, int *rowmap, double *band,
                                                        size_t mstride)
  {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= npad)
      return;
    if (r >= n)
      {
        if (blockIdx.y == 0)
          rowmap[r] = -1;
        band[blockIdx.y * mstride + (size_t)(r / FB) * (bb + 1) * FT + (size_t)(r % FB) * FB + r % FB] = 1.0;
        return;
      }
    if (blockIdx.y != 0)
      return;
    const int s = G.spacedim, cell = r / s, d = r - cell * s;
    rowmap[r]   = (int)grid_pid(G, cell % G.N, cell / G.N) * s + d;
  }

  // the lower triangle of the block rows into the zeroed band: entry ((p, d), (q, e)) with r(q, e) <= r(p, d).  One thread
  // per (word t, member k), k fastest as in the ensemble matrix: word t of member k is values[t ld_m + k]
  __global__ __launch_bounds__(256) void k_factor_scatter(const SlodGrid G, int NP, int cap, int bb, int n_members,
                                                         const double *__restrict__ values, size_t ld_m,
                                                         const uint32_t *__restrict__ cols, double *band, size_t mstride)
  {
    const int    s = G.spacedim;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x, t = w / n_members, k = w - t * n_members;
    if (t >= (size_t)NP * cap * s * s)
      return;
    const size_t   slot = t / (s * s);
    const int      de = (int)(t - slot * s * s), d = de / s, e = de - d * s;
    const uint32_t p = (uint32_t)(slot / cap), q = cols[slot];
    if (q >= (uint32_t)NP)
      return;
    const int r = factor_index(G, p, d), c = factor_index(G, q, e);
    const int I = r / FB, kb = I - c / FB;
    if (c > r || kb > bb)
      return;
    band[k * mstride + ((size_t)I * (bb + 1) + kb) * FT + (size_t)(c % FB) * FB + r % FB] = values[t * ld_m + k];
  }

  // Block column K of the factorisation; block x = block row r = K + x.  status[0]: the index of the first pivot that is
  // not > 0, or -1; a column after a failed one does nothing.  The factored diagonal tile goes to diag[K], not over A_KK in
  // the band: the other blocks of the launch read A_KK.  blockIdx.y = the member: its copy of the storage (mstride doubles
  // from the last) and its status word, nothing of another member.
  __global__ __launch_bounds__(64) void k_factor_column(int K, int bb, double *band, double *diag, double *piv, double *dinv,
                                                       int *status, size_t mstride)
  {
    __shared__ double sD[FB][FB + 1], sT[FB][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, piv += blockIdx.y * mstride, dinv += blockIdx.y * mstride;
    status += blockIdx.y;
    const int bad = status[0];
    if (bad >= 0 && bad < K * FB) // set by an earlier launch: the same answer in every block
      return;
    const int    lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int    r = K + blockIdx.x, J0 = max(0, K - bb), Jr = max(0, r - bb);
    const size_t ldb = (size_t)(bb + 1) * FT;
    auto         tile = [&](int I, int J) { return band + (size_t)I * ldb + (size_t)(I - J) * FT; };
    // accumulator layout: lane holds D[lk + 4 q][li]
    double4_t     accD, accT;
    const double *aD = tile(K, K), *aT = tile(r, K);
    for (int q = 0; q < 4; ++q)
      {
        accD[q] = aD[li * FB + lk + 4 * q];
        accT[q] = aT[li * FB + lk + 4 * q];
      }
    for (int J = J0; J < K; ++J)
      {
        const double *lk_ = tile(K, J);
        double        bk[4];
        for (int kk = 0; kk < 4; ++kk)
          bk[kk] = lk_[(4 * kk + lk) * FB + li]; // B[k][j] = L_KJ[j][k]; as an A operand the same word is L_KJ[i][k]
        for (int kk = 0; kk < 4; ++kk)
          accD = mfma(-bk[kk], bk[kk], accD);
        if (r != K && J >= Jr)
          {
            const double *lr = tile(r, J);
            for (int kk = 0; kk < 4; ++kk)
              accT = mfma(-lr[(4 * kk + lk) * FB + li], bk[kk], accT);
          }
      }
    for (int q = 0; q < 4; ++q)
      {
        sD[lk + 4 * q][li] = accD[q];
        sT[lk + 4 * q][li] = accT[q];
      }
    __syncthreads();
    // Cholesky of the diagonal tile, lower triangle of sD in place; the reciprocal diagonal goes to sD[j][FB]
    for (int j = 0; j < FB; ++j)
      {
        const double p = sD[j][j];
        const bool   ok = p > 0.0; // false for NaN too
        const double dj = sqrt(ok ? p : 1.0);
        __syncthreads();
        if (lane == 0)
          {
            sD[j][j]  = dj;
            sD[j][FB] = 1.0 / dj;
            if (blockIdx.x == 0)
              {
                piv[K * FB + j] = p;
                if (!ok && status[0] < 0)
                  status[0] = K * FB + j;
              }
          }
        else if (lane > j && lane < FB)
          sD[lane][j] = sD[lane][j] / dj;
        __syncthreads();
        for (int idx = lane; idx < FT; idx += 64)
          {
            const int i = idx >> 4, c = idx & 15;
            if (c > j && i >= c)
              sD[i][c] = fma(-sD[i][j], sD[c][j], sD[i][c]);
          }
        __syncthreads();
      }
    double *out = blockIdx.x == 0 ? diag + (size_t)K * FT : tile(r, K);
    if (blockIdx.x == 0)
      {
        for (int idx = lane; idx < FT; idx += 64)
          {
            const int c = idx >> 4, i = idx & 15;
            out[idx]    = i >= c ? sD[i][c] : 0.0;
          }
        if (lane < FB)
          dinv[K * FB + lane] = sD[lane][FB];
        return;
      }
    // L_rK L_KK^T = T by rows: lane i < 16 holds row i
    if (lane < FB)
      {
        double x[FB];
#pragma unroll
        for (int j = 0; j < FB; ++j)
          {
            double v = sT[lane][j];
#pragma unroll
            for (int m = 0; m < j; ++m)
              v = fma(-x[m], sD[j][m], v);
            x[j] = v * sD[j][FB];
          }
#pragma unroll
        for (int j = 0; j < FB; ++j)
          sT[lane][j] = x[j];
      }
    __syncthreads();
    for (int idx = lane; idx < FT; idx += 64)
      out[idx] = sT[idx & 15][idx >> 4];
  }

  // Block column K of  S = L D L^T  (L unit lower triangular, D diagonal, 1 x 1 pivots, no pivoting: a permutation would
  // destroy the band and the tiles): the launch shape, the operands and the storage of k_factor_column.  Block K + x forms
  // T = A_rK - sum_J L_rJ D_J L_KJ^T  with the B operand scaled by D_J (piv of the earlier columns), factors the diagonal
  // tile in LDS without a square root and solves  L_rK = T L_KK^-T D_K^-1  by rows.  diag[K]: L_KK with its unit diagonal,
  // piv: D (signed), dinv: 1 / D.  status[0]: the index of the first pivot that is zero, infinite or NaN, or -1.
  __global__ __launch_bounds__(64) void k_ldl_column(int K, int bb, double *band, double *diag, double *piv, double *dinv, int *status,
                                                    size_t mstride)
  {
    __shared__ double sD[FB][FB + 1], sT[FB][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, piv += blockIdx.y * mstride, dinv += blockIdx.y * mstride;
    status += blockIdx.y;
    const int bad = status[0];
    if (bad >= 0 && bad < K * FB) // set by an earlier launch: the same answer in every block
      return;
    const int    lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int    r = K + blockIdx.x, J0 = max(0, K - bb), Jr = max(0, r - bb);
    const size_t ldb = (size_t)(bb + 1) * FT;
    auto         tile = [&](int I, int J) { return band + (size_t)I * ldb + (size_t)(I - J) * FT; };
    // accumulator layout: lane holds D[lk + 4 q][li]
    double4_t     accD, accT;
    const double *aD = tile(K, K), *aT = tile(r, K);
    for (int q = 0; q < 4; ++q)
      {
        accD[q] = aD[li * FB + lk + 4 * q];
        accT[q] = aT[li * FB + lk + 4 * q];
      }
    for (int J = J0; J < K; ++J)
      {
        const double *lk_ = tile(K, J), *dJ = piv + J * FB;
        double        ak[4], bk[4];
        for (int kk = 0; kk < 4; ++kk)
          {
            ak[kk] = lk_[(4 * kk + lk) * FB + li]; // as an A operand L_KJ[i][k], as a B operand L_KJ[j][k]
            bk[kk] = ak[kk] * dJ[4 * kk + lk];     // B[k][j] = D_J[k] L_KJ[j][k]
          }
        for (int kk = 0; kk < 4; ++kk)
          accD = mfma(-ak[kk], bk[kk], accD);
        if (r != K && J >= Jr)
          {
            const double *lr = tile(r, J);
            for (int kk = 0; kk < 4; ++kk)
              accT = mfma(-lr[(4 * kk + lk) * FB + li], bk[kk], accT);
          }
      }
    for (int q = 0; q < 4; ++q)
      {
        sD[lk + 4 * q][li] = accD[q];
        sT[lk + 4 * q][li] = accT[q];
      }
    __syncthreads();
    // L D L^T of the diagonal tile: column j of L goes to the lower triangle of sD, the unscaled column w = L d_j to row j of
    // the upper triangle (the update of entry (i, c) is w_i L_cj), the reciprocal pivot to sD[j][FB]
    for (int j = 0; j < FB; ++j)
      {
        const double p = sD[j][j];
        // zero, infinite and NaN fail; every comparison is false for NaN
        const bool   ok = (p > 0.0 && p < HUGE_VAL) || (p < 0.0 && p > -HUGE_VAL);
        double       dj;
        if (ok)
          dj = p;
        else
          dj = 1.0;
        __syncthreads();
        if (lane == 0)
          {
            sD[j][FB] = 1.0 / dj;
            if (blockIdx.x == 0)
              {
                piv[K * FB + j] = p;
                if (!ok)
                  {
                    if (status[0] < 0)
                      status[0] = K * FB + j;
                  }
              }
          }
        else if (lane > j && lane < FB)
          {
            const double w = sD[lane][j];
            sD[j][lane]    = w;
            sD[lane][j]    = w / dj;
          }
        __syncthreads();
        for (int idx = lane; idx < FT; idx += 64)
          {
            const int i = idx >> 4, c = idx & 15;
            if (c > j && i >= c)
              sD[i][c] = fma(-sD[j][i], sD[c][j], sD[i][c]);
          }
        __syncthreads();
      }
    double *out = blockIdx.x == 0 ? diag + (size_t)K * FT : tile(r, K);
    if (blockIdx.x == 0)
      {
        for (int idx = lane; idx < FT; idx += 64)
          {
            const int c = idx >> 4, i = idx & 15;
            out[idx]    = i > c ? sD[i][c] : (i == c ? 1.0 : 0.0);
          }
        if (lane < FB)
          dinv[K * FB + lane] = sD[lane][FB];
        return;
      }
    // L_rK D_K L_KK^T = T by rows: lane i < 16 holds row i; y = T L_KK^-T, then the row is scaled by 1 / D_K
    if (lane < FB)
      {
        double y[FB];
#pragma unroll
        for (int j = 0; j < FB; ++j)
          {
            double v = sT[lane][j];
#pragma unroll
            for (int m = 0; m < j; ++m)
              v = fma(-y[m], sD[j][m], v);
            y[j] = v;
          }
#pragma unroll
        for (int j = 0; j < FB; ++j)
          sT[lane][j] = y[j] * sD[j][FB];
      }
    __syncthreads();
    for (int idx = lane; idx < FT; idx += 64)
      out[idx] = sT[idx & 15][idx >> 4];
  }

  // The row sums behind the two norms of an LDL^T factor, in factor order: block row (or column) blockIdx.x of member
  // blockIdx.y, entry i of it on thread (i = tid & 15, part = tid >> 4), which adds the tiles k = part, part + 16, .. in
  // ascending k and ascending position; the 16 parts are then added in ascending order: fixed sums.
  //   MODE 0, after k_factor_scatter:  out[r] = sum_c |S_rc|, S the symmetric matrix whose lower triangle is in the band
  //   MODE 1, after the last column:   out[c] = |D_c| sum_r |L_rc|            = (|D| (|L^T| e))_c
  //   MODE 2:                          out[r] = sum_c |L_rc| in[c]            = (|L| (|D| (|L^T| e)))_r
  // k_ldl_norm_max takes the maximum over the n real rows (the padding rows and columns add nothing to a real row).
  template <int MODE>
  __global__ __launch_bounds__(256) void k_ldl_norms(int nb, int bb, const double *__restrict__ band, const double *__restrict__ diag,
                                                    const double *__restrict__ piv, const double *__restrict__ in, double *__restrict__ out,
                                                    size_t mstride)
  {
    __shared__ double sP[16][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, piv += blockIdx.y * mstride, out += blockIdx.y * mstride;
    if (MODE == 2) // (the other modes read no vector: in is NULL)
      in += blockIdx.y * mstride;
    const int     I = blockIdx.x, tid = threadIdx.x, i = tid & 15, part = tid >> 4;
    const size_t  ldb = (size_t)(bb + 1) * FT;
    // the diagonal tile: the band's for S (lower triangle; the padding has its unit diagonal), L_II with its unit diagonal
    const double *dtile = MODE == 0 ? band + (size_t)I * ldb : diag + (size_t)I * FT;
    auto          reduce = [&](double acc) { // the 16 parts of entry i in ascending order; the sum is valid for tid < 16
      __syncthreads();
      sP[part][i] = acc;
      __syncthreads();
      double v = 0.0;
      if (tid < FB)
        for (int q = 0; q < 16; ++q)
          v += sP[q][tid];
      return v;
    };
    double v = 0.0;
    if (MODE != 1) // row i of the block row: the tiles (I, I - k), of the diagonal tile the columns up to the diagonal
      {
        double acc = 0.0;
        for (int k = part; k <= min(bb, I); k += 16)
          {
            const double *t = k == 0 ? dtile : band + (size_t)I * ldb + (size_t)k * FT;
            for (int c = 0; c < (k == 0 ? i + 1 : FB); ++c)
              acc += fabs(t[c * FB + i]) * (MODE == 2 ? in[(I - k) * FB + c] : 1.0);
          }
        v += reduce(acc);
      }
    if (MODE != 2) // column i of the block column: the tiles (I + k, I), of the diagonal tile the rows below the diagonal
      {            // (S: the transposed half of the row) or from it (L: the whole column)
        double acc = 0.0;
        for (int k = part; k <= min(bb, nb - 1 - I); k += 16)
          {
            const double *t = k == 0 ? dtile : band + (size_t)(I + k) * ldb + (size_t)k * FT;
            for (int r = k == 0 ? (MODE == 1 ? i : i + 1) : 0; r < FB; ++r)
              acc += fabs(t[i * FB + r]);
          }
        v += reduce(acc);
      }
    if (tid < FB)
      out[I * FB + tid] = MODE == 1 ? fabs(piv[I * FB + tid]) * v : v;
  }

  // out[0] = max_{r < n} v[r] per member (blockIdx.y); a maximum does not depend on the order it is taken in
  __global__ __launch_bounds__(256) void k_ldl_norm_max(int n, const double *__restrict__ v, double *__restrict__ out, size_t mstride)
  {
    __shared__ double sM[256];
    v += blockIdx.y * mstride, out += blockIdx.y * mstride;
    double best = 0.0;
    for (int r = threadIdx.x; r < n; r += 256)
      best = fmax(best, v[r]);
    sM[threadIdx.x] = best;
    __syncthreads();
    if (threadIdx.x == 0)
      {
        for (int q = 1; q < 256; ++q)
          best = fmax(best, sM[q]);
        out[0] = best;
      }
  }

  // Both sweeps for the 16 columns from blockIdx.x * 16 of the window of member blockIdx.y: its n_rhs columns from
  // blockIdx.y * n_rhs, on its copy of the factor.  rhs and u may be the same array: a block row of rhs is read before the
  // same rows of u are written, and a block touches its own columns only.  LDL: the sweeps on a factor of k_ldl_column,
  // L y = b with the unit diagonal, then L^T x = D^-1 y: the block row of y is scaled by 1 / D as the backward sweep loads it.
  template <bool LDL>
  __global__ __launch_bounds__(256) void k_factor_solve(int nb, int bb, const double *__restrict__ band, const double *__restrict__ diag,
                                                       const double *__restrict__ dinv, size_t mstride, const int *__restrict__ rowmap,
                                                       int n_rhs, const double *rhs, size_t ld_rhs, double *u, size_t ld_u)
  {
    __shared__ double sP[4][FB][FB + 1], sL[FB][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, dinv += blockIdx.y * mstride;
    rhs += (size_t)blockIdx.y * n_rhs, u += (size_t)blockIdx.y * n_rhs;
    const int         tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int         c0 = blockIdx.x * FB;
    const bool        col_ok = c0 + li < n_rhs;
    const size_t      ldb = (size_t)(bb + 1) * FT;
    // entry (row 16 I + i, this lane's column) of a multi-vector; padding rows and columns read as 0
    auto load = [&](const double *x, size_t ld, int I, int i) {
      const int row = rowmap[I * FB + i];
      return col_ok && row >= 0 ? x[(size_t)row * ld + c0 + li] : 0.0;
    };
    for (int sweep = 0; sweep < 2; ++sweep)
      for (int step = 0; step < nb; ++step)
        {
          const int     I = sweep == 0 ? step : nb - 1 - step;
          const int     nk = sweep == 0 ? min(bb, I) : min(bb, nb - 1 - I); // tiles left (right, transposed) of the diagonal
          const double *src = sweep == 0 ? rhs : u;
          const size_t  ld_src = sweep == 0 ? ld_rhs : ld_u;
          double4_t     acc = {0.0, 0.0, 0.0, 0.0};
          if (wave == 0)
            for (int q = 0; q < 4; ++q)
              acc[q] = LDL && sweep == 1 ? load(src, ld_src, I, lk + 4 * q) * dinv[I * FB + lk + 4 * q] : load(src, ld_src, I, lk + 4 * q);
          for (int k = 1 + wave; k <= nk; k += 4)
            {
              // forward: tile (I, I - k) times X_{I-k}; backward: tile (I + k, I) transposed times X_{I+k}
              const int     X = sweep == 0 ? I - k : I + k;
              const double *t = band + (size_t)(sweep == 0 ? I : X) * ldb + (size_t)k * FT;
              for (int kk = 0; kk < 4; ++kk)
                {
                  const double a = sweep == 0 ? t[(4 * kk + lk) * FB + li] : t[li * FB + 4 * kk + lk];
                  acc            = mfma(-a, load(u, ld_u, X, 4 * kk + lk), acc);
                }
            }
          for (int q = 0; q < 4; ++q)
            sP[wave][lk + 4 * q][li] = acc[q];
          sL[tid >> 4][tid & 15] = diag[(size_t)I * FT + (size_t)(tid & 15) * FB + (tid >> 4)]; // sL[r][c] = L_II[r][c]
          __syncthreads();
          if (tid < FB)
            {
              double x[FB];
#pragma unroll
              for (int i = 0; i < FB; ++i)
                x[i] = ((sP[0][i][tid] + sP[1][i][tid]) + sP[2][i][tid]) + sP[3][i][tid];
              if (sweep == 0)
                {
#pragma unroll
                  for (int i = 0; i < FB; ++i)
                    {
                      double v = x[i];
#pragma unroll
                      for (int m = 0; m < i; ++m)
                        v = fma(-sL[i][m], x[m], v);
                      x[i] = LDL ? v : v * dinv[I * FB + i];
                    }
                }
              else
                {
#pragma unroll
                  for (int i = FB - 1; i >= 0; --i)
                    {
                      double v = x[i];
#pragma unroll
                      for (int m = FB - 1; m > i; --m)
                        v = fma(-sL[m][i], x[m], v);
                      x[i] = LDL ? v : v * dinv[I * FB + i];
                    }
                }
              if (c0 + tid < n_rhs)
                {
#pragma unroll
                  for (int i = 0; i < FB; ++i)
                    {
                      const int row = rowmap[I * FB + i];
                      if (row >= 0)
                        u[(size_t)row * ld_u + c0 + tid] = x[i];
                    }
                }
            }
          __syncthreads(); // the rows of X just written are read by all waves in the next steps
        }
  }

  // ---------------------------------------------------------------------------------
  // The complex symmetric factor  S_k = alpha_k A + beta_k B = L D L^T  (plain transpose, no conjugate; kind
  // SLOD_FACTOR_ZLDL): the twins of the kernels above on two planes, real and imaginary, of every array.
  // ---------------------------------------------------------------------------------
  // 1 / (dr + i di) by Smith's formula: no square of a part is formed.  di = 0 gives (1 / dr, 0).
  __device__ __forceinline__ void zrecip(double dr, double di, double &ir, double &ii)
  {
    if (fabs(dr) >= fabs(di))
      {
        const double t = di / dr, den = fma(di, t, dr);
        ir = 1.0 / den, ii = -t / den;
      }
    else
      {
        const double t = dr / di, den = fma(dr, t, di);
        ir = t / den, ii = -1.0 / den;
      }
  }
  // (cr, ci) -= (ar + i ai) (br + i bi), four fma in one order
  __device__ __forceinline__ void zfms(double ar, double ai, double br, double bi, double &cr, double &ci)
  {
    cr = fma(-ar, br, cr);
    cr = fma(ai, bi, cr);
    ci = fma(-ar, bi, ci);
    ci = fma(-ai, br, ci);
  }
  // (ar + i ai) (br + i bi): a product and an fma per part
  __device__ __forceinline__ void zmul(double ar, double ai, double br, double bi, double &cr, double &ci)
  {
    cr = fma(-ai, bi, ar * br);
    ci = fma(ar, bi, ai * br);
  }
  // C -= A B on complex tiles: four v_mfma_f64_16x16x4_f64 into the two accumulators, in this order
  __device__ __forceinline__ void zmfma(double ar, double ai, double br, double bi, double4_t &cr, double4_t &ci)
  {
    cr = mfma(-ar, br, cr);
    cr = mfma(ai, bi, cr);
    ci = mfma(-ar, bi, ci);
    ci = mfma(-ai, br, ci);
  }

  // k_factor_scatter for the combination: word t of member k is  (alpha_re a + beta_re b, alpha_im a + beta_im b),  every
  // product and every sum rounded on its own.  coef: [n_members][4].  a, b: ensemble matrices of kmat members (entry t of
  // member m at a[t ld_a + m]); factor member k is the flat member j = j0 + k of a (coefficient, matrix) table and reads
  // matrix member j % kmat.  One matrix each for all members is the launch kmat = 1, ld_a = ld_b = 1.
  // THREE: a third term gamma_k c (slod_lod_factor_create_zldl3), coef_c: [n_members][2]; the word is
  // ((alpha_re a + beta_re b) + gamma_re c, (alpha_im a + beta_im b) + gamma_im c), rounded the same way.
  template <bool THREE>
  __global__ __launch_bounds__(256) void k_zfactor_scatter(const SlodGrid G, int NP, int cap, int bb, int n_members,
                                                          const double *__restrict__ a, size_t ld_a, const double *__restrict__ b,
                                                          size_t ld_b, const double *__restrict__ c3, size_t ld_c, int kmat, size_t j0,
                                                          const double *__restrict__ coef, const double *__restrict__ coef_c,
                                                          const uint32_t *__restrict__ cols, double *band, size_t im_band,
                                                          size_t mstride)
  {
#pragma clang fp contract(off)
    const int    s = G.spacedim;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x, t = w / n_members, k = w - t * n_members;
    if (t >= (size_t)NP * cap * s * s)
      return;
    const size_t   slot = t / (s * s);
    const int      de = (int)(t - slot * s * s), d = de / s, e = de - d * s;
    const uint32_t p = (uint32_t)(slot / cap), q = cols[slot];
    if (q >= (uint32_t)NP)
      return;
    const int r = factor_index(G, p, d), c = factor_index(G, q, e);
    const int I = r / FB, kb = I - c / FB;
    if (c > r || kb > bb)
      return;
    const double *ck = coef + 4 * k;
    const size_t  m = (j0 + k) % (size_t)kmat;
    const double  av = a[t * ld_a + m], bv = b[t * ld_b + m];
    const double  re_a = ck[0] * av, re_b = ck[2] * bv, im_a = ck[1] * av, im_b = ck[3] * bv;
    double       *out = band + k * mstride + ((size_t)I * (bb + 1) + kb) * FT + (size_t)(c % FB) * FB + r % FB;
    if constexpr (THREE)
      {
        const double cv = c3[t * ld_c + m];
        const double re_c = coef_c[2 * k] * cv, im_c = coef_c[2 * k + 1] * cv;
        const double re = re_a + re_b, im = im_a + im_b;
        out[0]       = re + re_c;
        out[im_band] = im + im_c;
      }
    else
      {
        out[0]       = re_a + re_b;
        out[im_band] = im_a + im_b;
      }
  }

  // Block column K of the complex  S = L D L^T:  the launch shape, the operands and the storage of k_ldl_column, every
  // array in two planes (im_band, im_diag, im_vec doubles from the real one to the imaginary one).  The update
  // T -= L_rJ D_J L_KJ^T  uses the plain transpose; a pivot fails when both parts are zero or a part is not finite.
  __global__ __launch_bounds__(64) void k_zldl_column(int K, int bb, double *band, size_t im_band, double *diag, size_t im_diag,
                                                     double *piv, double *dinv, size_t im_vec, int *status, size_t mstride)
  {
    __shared__ double sDr[FB][FB + 1], sDi[FB][FB + 1], sTr[FB][FB + 1], sTi[FB][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, piv += blockIdx.y * mstride, dinv += blockIdx.y * mstride;
    status += blockIdx.y;
    const int bad = status[0];
    if (bad >= 0 && bad < K * FB) // set by an earlier launch: the same answer in every block
      return;
    const int    lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int    r = K + blockIdx.x, J0 = max(0, K - bb), Jr = max(0, r - bb);
    const size_t ldb = (size_t)(bb + 1) * FT;
    auto         tile = [&](int I, int J) { return band + (size_t)I * ldb + (size_t)(I - J) * FT; };
    // accumulator layout: lane holds D[lk + 4 q][li]
    double4_t     accDr, accDi, accTr, accTi;
    const double *aD = tile(K, K), *aT = tile(r, K);
    for (int q = 0; q < 4; ++q)
      {
        const int at = li * FB + lk + 4 * q;
        accDr[q] = aD[at], accDi[q] = aD[im_band + at];
        accTr[q] = aT[at], accTi[q] = aT[im_band + at];
      }
    for (int J = J0; J < K; ++J)
      {
        const double *lk_ = tile(K, J), *dJ = piv + J * FB;
        double        akr[4], aki[4], bkr[4], bki[4];
        for (int kk = 0; kk < 4; ++kk)
          {
            const int at = (4 * kk + lk) * FB + li; // as an A operand L_KJ[i][k], as a B operand L_KJ[j][k]
            akr[kk] = lk_[at], aki[kk] = lk_[im_band + at];
            zmul(akr[kk], aki[kk], dJ[4 * kk + lk], dJ[im_vec + 4 * kk + lk], bkr[kk], bki[kk]); // B[k][j] = D_J[k] L_KJ[j][k]
          }
        for (int kk = 0; kk < 4; ++kk)
          zmfma(akr[kk], aki[kk], bkr[kk], bki[kk], accDr, accDi);
        if (r != K && J >= Jr)
          {
            const double *lr = tile(r, J);
            for (int kk = 0; kk < 4; ++kk)
              {
                const int at = (4 * kk + lk) * FB + li;
                zmfma(lr[at], lr[im_band + at], bkr[kk], bki[kk], accTr, accTi);
              }
          }
      }
    for (int q = 0; q < 4; ++q)
      {
        sDr[lk + 4 * q][li] = accDr[q], sDi[lk + 4 * q][li] = accDi[q];
        sTr[lk + 4 * q][li] = accTr[q], sTi[lk + 4 * q][li] = accTi[q];
      }
    __syncthreads();
    // L D L^T of the diagonal tile as in k_ldl_column: column j of L to the lower triangle of sD, the unscaled column
    // w = L d_j to row j of the upper triangle, the reciprocal pivot to sD[j][FB]
    for (int j = 0; j < FB; ++j)
      {
        const double pr = sDr[j][j], pi = sDi[j][j];
        // both parts zero, or a part infinite or NaN, fails; every comparison is false for NaN
        const bool   finite = fabs(pr) < HUGE_VAL && fabs(pi) < HUGE_VAL;
        const bool   ok = finite && (pr != 0.0 || pi != 0.0);
        double       ir, ii;
        if (ok)
          zrecip(pr, pi, ir, ii);
        else
          ir = 1.0, ii = 0.0;
        __syncthreads();
        if (lane == 0)
          {
            sDr[j][FB] = ir, sDi[j][FB] = ii;
            if (blockIdx.x == 0)
              {
                piv[K * FB + j] = pr, piv[im_vec + K * FB + j] = pi;
                if (!ok)
                  {
                    if (status[0] < 0)
                      status[0] = K * FB + j;
                  }
              }
          }
        else if (lane > j && lane < FB)
          {
            const double wr = sDr[lane][j], wi = sDi[lane][j];
            sDr[j][lane] = wr, sDi[j][lane] = wi;
            zmul(wr, wi, ir, ii, sDr[lane][j], sDi[lane][j]);
          }
        __syncthreads();
        for (int idx = lane; idx < FT; idx += 64)
          {
            const int i = idx >> 4, c = idx & 15;
            if (c > j && i >= c)
              zfms(sDr[j][i], sDi[j][i], sDr[c][j], sDi[c][j], sDr[i][c], sDi[i][c]);
          }
        __syncthreads();
      }
    if (blockIdx.x == 0)
      {
        double *out = diag + (size_t)K * FT;
        for (int idx = lane; idx < FT; idx += 64)
          {
            const int c = idx >> 4, i = idx & 15;
            out[idx]           = i > c ? sDr[i][c] : (i == c ? 1.0 : 0.0);
            out[im_diag + idx] = i > c ? sDi[i][c] : 0.0;
          }
        if (lane < FB)
          dinv[K * FB + lane] = sDr[lane][FB], dinv[im_vec + K * FB + lane] = sDi[lane][FB];
        return;
      }
    // L_rK D_K L_KK^T = T by rows: lane i < 16 holds row i; y = T L_KK^-T, then the row is scaled by 1 / D_K
    if (lane < FB)
      {
        double yr[FB], yi[FB];
#pragma unroll
        for (int j = 0; j < FB; ++j)
          {
            double vr = sTr[lane][j], vi = sTi[lane][j];
#pragma unroll
            for (int m = 0; m < j; ++m)
              zfms(yr[m], yi[m], sDr[j][m], sDi[j][m], vr, vi);
            yr[j] = vr, yi[j] = vi;
          }
#pragma unroll
        for (int j = 0; j < FB; ++j)
          zmul(yr[j], yi[j], sDr[j][FB], sDi[j][FB], sTr[lane][j], sTi[lane][j]);
      }
    __syncthreads();
    double *out = tile(r, K);
    for (int idx = lane; idx < FT; idx += 64)
      out[idx] = sTr[idx & 15][idx >> 4], out[im_band + idx] = sTi[idx & 15][idx >> 4];
  }

  // k_ldl_norms with moduli: the same threads, tiles and orders of summation on |z| = hypot(re, im) of the two planes.
  // piv, in and out are real vectors but for piv's imaginary plane, im_vec behind it.
  template <int MODE>
  __global__ __launch_bounds__(256) void k_zldl_norms(int nb, int bb, const double *__restrict__ band, size_t im_band,
                                                     const double *__restrict__ diag, size_t im_diag, const double *__restrict__ piv,
                                                     size_t im_vec, const double *__restrict__ in, double *__restrict__ out,
                                                     size_t mstride)
  {
    __shared__ double sP[16][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, piv += blockIdx.y * mstride, out += blockIdx.y * mstride;
    if (MODE == 2) // (the other modes read no vector: in is NULL)
      in += blockIdx.y * mstride;
    const int     I = blockIdx.x, tid = threadIdx.x, i = tid & 15, part = tid >> 4;
    const size_t  ldb = (size_t)(bb + 1) * FT;
    const double *dtile = MODE == 0 ? band + (size_t)I * ldb : diag + (size_t)I * FT;
    const size_t  im_dtile = MODE == 0 ? im_band : im_diag;
    auto          reduce = [&](double acc) { // the 16 parts of entry i in ascending order; the sum is valid for tid < 16
      __syncthreads();
      sP[part][i] = acc;
      __syncthreads();
      double v = 0.0;
      if (tid < FB)
        for (int q = 0; q < 16; ++q)
          v += sP[q][tid];
      return v;
    };
    double v = 0.0;
    if (MODE != 1)
      {
        double acc = 0.0;
        for (int k = part; k <= min(bb, I); k += 16)
          {
            const double *t = k == 0 ? dtile : band + (size_t)I * ldb + (size_t)k * FT;
            const size_t  im = k == 0 ? im_dtile : im_band;
            for (int c = 0; c < (k == 0 ? i + 1 : FB); ++c)
              acc += hypot(t[c * FB + i], t[im + c * FB + i]) * (MODE == 2 ? in[(I - k) * FB + c] : 1.0);
          }
        v += reduce(acc);
      }
    if (MODE != 2)
      {
        double acc = 0.0;
        for (int k = part; k <= min(bb, nb - 1 - I); k += 16)
          {
            const double *t = k == 0 ? dtile : band + (size_t)(I + k) * ldb + (size_t)k * FT;
            const size_t  im = k == 0 ? im_dtile : im_band;
            for (int r = k == 0 ? (MODE == 1 ? i : i + 1) : 0; r < FB; ++r)
              acc += hypot(t[i * FB + r], t[im + i * FB + r]);
          }
        v += reduce(acc);
      }
    if (tid < FB)
      out[I * FB + tid] = MODE == 1 ? hypot(piv[I * FB + tid], piv[im_vec + I * FB + tid]) * v : v;
  }

  // The two sweeps of k_factor_solve<true> on a complex factor: the same deal of tiles to waves and the same order of
  // summation, a complex tile product per tile.  rhs_im NULL: a real load.  Member blockIdx.y of the launch reads the
  // rhs columns ((rhs_first + blockIdx.y) % rhs_members) n_rhs .. and writes the columns blockIdx.y n_rhs .. of u:
  // period 1 is the shared rhs, a period of at least the members launched (rhs_first = 0) a rhs of their own each.
  __global__ __launch_bounds__(256) void k_zfactor_solve(int nb, int bb, const double *__restrict__ band, size_t im_band,
                                                        const double *__restrict__ diag, size_t im_diag,
                                                        const double *__restrict__ dinv, size_t im_vec, size_t mstride,
                                                        const int *__restrict__ rowmap, int n_rhs, int rhs_first, int rhs_members,
                                                        const double *rhs_re, const double *rhs_im, size_t ld_rhs, double *u_re,
                                                        double *u_im, size_t ld_u)
  {
    __shared__ double sPr[4][FB][FB + 1], sPi[4][FB][FB + 1], sLr[FB][FB + 1], sLi[FB][FB + 1];
    band += blockIdx.y * mstride, diag += blockIdx.y * mstride, dinv += blockIdx.y * mstride;
    {
      const size_t base = (size_t)(((unsigned)rhs_first + blockIdx.y) % (unsigned)rhs_members) * n_rhs;
      rhs_re += base;
      if (rhs_im)
        rhs_im += base;
    }
    u_re += (size_t)blockIdx.y * n_rhs, u_im += (size_t)blockIdx.y * n_rhs;
    const int    tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int    c0 = blockIdx.x * FB;
    const bool   col_ok = c0 + li < n_rhs;
    const size_t ldb = (size_t)(bb + 1) * FT;
    // entry (row 16 I + i, this lane's column) of a multi-vector; padding rows and columns, and a NULL plane, read as 0
    auto load = [&](const double *x, size_t ld, int I, int i) {
      const int row = rowmap[I * FB + i];
      return x && col_ok && row >= 0 ? x[(size_t)row * ld + c0 + li] : 0.0;
    };
    for (int sweep = 0; sweep < 2; ++sweep)
      for (int step = 0; step < nb; ++step)
        {
          const int     I = sweep == 0 ? step : nb - 1 - step;
          const int     nk = sweep == 0 ? min(bb, I) : min(bb, nb - 1 - I); // tiles left (right, transposed) of the diagonal
          double4_t     accr = {0.0, 0.0, 0.0, 0.0}, acci = {0.0, 0.0, 0.0, 0.0};
          if (wave == 0)
            for (int q = 0; q < 4; ++q)
              {
                const int i = lk + 4 * q;
                if (sweep == 0)
                  accr[q] = load(rhs_re, ld_rhs, I, i), acci[q] = load(rhs_im, ld_rhs, I, i);
                else // y scaled by 1 / D as the backward sweep loads it
                  {
                    double vr, vi;
                    zmul(load(u_re, ld_u, I, i), load(u_im, ld_u, I, i), dinv[I * FB + i], dinv[im_vec + I * FB + i], vr, vi);
                    accr[q] = vr, acci[q] = vi;
                  }
              }
          for (int k = 1 + wave; k <= nk; k += 4)
            {
              // forward: tile (I, I - k) times X_{I-k}; backward: tile (I + k, I) transposed times X_{I+k}
              const int     X = sweep == 0 ? I - k : I + k;
              const double *t = band + (size_t)(sweep == 0 ? I : X) * ldb + (size_t)k * FT;
              for (int kk = 0; kk < 4; ++kk)
                {
                  const int at = sweep == 0 ? (4 * kk + lk) * FB + li : li * FB + 4 * kk + lk;
                  zmfma(t[at], t[im_band + at], load(u_re, ld_u, X, 4 * kk + lk), load(u_im, ld_u, X, 4 * kk + lk), accr, acci);
                }
            }
          for (int q = 0; q < 4; ++q)
            sPr[wave][lk + 4 * q][li] = accr[q], sPi[wave][lk + 4 * q][li] = acci[q];
          {
            const size_t at = (size_t)I * FT + (size_t)(tid & 15) * FB + (tid >> 4); // sL[r][c] = L_II[r][c]
            sLr[tid >> 4][tid & 15] = diag[at], sLi[tid >> 4][tid & 15] = diag[im_diag + at];
          }
          __syncthreads();
          if (tid < FB)
            {
              double xr[FB], xi[FB];
#pragma unroll
              for (int i = 0; i < FB; ++i)
                {
                  xr[i] = ((sPr[0][i][tid] + sPr[1][i][tid]) + sPr[2][i][tid]) + sPr[3][i][tid];
                  xi[i] = ((sPi[0][i][tid] + sPi[1][i][tid]) + sPi[2][i][tid]) + sPi[3][i][tid];
                }
              if (sweep == 0)
                {
#pragma unroll
                  for (int i = 0; i < FB; ++i)
#pragma unroll
                    for (int m = 0; m < i; ++m)
                      zfms(sLr[i][m], sLi[i][m], xr[m], xi[m], xr[i], xi[i]);
                }
              else
                {
#pragma unroll
                  for (int i = FB - 1; i >= 0; --i)
#pragma unroll
                    for (int m = FB - 1; m > i; --m)
                      zfms(sLr[m][i], sLi[m][i], xr[m], xi[m], xr[i], xi[i]);
                }
              if (c0 + tid < n_rhs)
                {
#pragma unroll
                  for (int i = 0; i < FB; ++i)
                    {
                      const int row = rowmap[I * FB + i];
                      if (row >= 0)
                        u_re[(size_t)row * ld_u + c0 + tid] = xr[i], u_im[(size_t)row * ld_u + c0 + tid] = xi[i];
                    }
                }
            }
          __syncthreads(); // the rows of X just written are read by all waves in the next steps
        }
  }
} // namespace

// what every consumer of a real factor answers to a complex one, behind the call's name
static const char COMPLEX_REFUSED[] = ": a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex";

void slod_lod_factor_solve_launch(const slod_lod_factor *f, hipStream_t st, const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u,
                                  size_t ld_u, int first_member, int n_members)
{
  const size_t first = (size_t)first_member * f->member_doubles;
  const dim3   grid((unsigned)((n_rhs + FB - 1) / FB), (unsigned)n_members);
  if (f->kind == SLOD_FACTOR_LDL)
    hipLaunchKernelGGL(k_factor_solve<true>, grid, dim3(256), 0, st, f->nb, f->bb, f->band + first, f->diag + first, f->dinv + first,
                       f->member_doubles, f->rowmap, n_rhs, d_rhs, ld_rhs, d_u, ld_u);
  else
    hipLaunchKernelGGL(k_factor_solve<false>, grid, dim3(256), 0, st, f->nb, f->bb, f->band + first, f->diag + first, f->dinv + first,
                       f->member_doubles, f->rowmap, n_rhs, d_rhs, ld_rhs, d_u, ld_u);
}

int slod_lod_factor_check(const slod_handle *h, const char *who, const slod_lod_factor *f, int n_members)
{
  if (!f)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL factor");
  if (f->h != h || f->n != h->NP * h->cfg.spacedim)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": factor of another handle / row count");
  if (f->kind == SLOD_FACTOR_ZLDL)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + COMPLEX_REFUSED);
  if (f->n_members != n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": factor of another member count");
  return SLOD_OK;
}

void slod_lod_zfactor_solve_launch(const slod_lod_factor *f, hipStream_t st, int first_member, int n_members, const double *d_rhs_re,
                                   const double *d_rhs_im, size_t ld_rhs, int n_rhs, int rhs_first, int rhs_members, double *d_u_re,
                                   double *d_u_im, size_t ld_u)
{
  const size_t first = (size_t)first_member * f->member_doubles;
  const dim3   grid((unsigned)((n_rhs + FB - 1) / FB), (unsigned)n_members);
  hipLaunchKernelGGL(k_zfactor_solve, grid, dim3(256), 0, st, f->nb, f->bb, f->band + first, f->im_band, f->diag + first, f->im_diag,
                     f->dinv + first, f->im_vec, f->member_doubles, f->rowmap, n_rhs, rhs_first, rhs_members, d_rhs_re, d_rhs_im,
                     ld_rhs, d_u_re, d_u_im, ld_u);
}

namespace
{
  constexpr int MAX_MEMBERS = 65535; // members sit on blockIdx.y

  // slod_lod_factor_create is the call with ld_m = 1, n_members = 1 and no bad_pivot; arguments are checked by the caller.
  // kind SLOD_FACTOR_LDL: the same storage with two norms behind a member's pivots and two work vectors behind its dinv,
  // k_ldl_column in place of k_factor_column, k_ldl_norms / k_ldl_norm_max before the first and after the last column.
  int factor_create(slod_handle *h, const char *who, bool ensemble, int kind, const double *d_values, size_t ld_m, int n_members,
                    const uint32_t *d_cols, int32_t *bad_pivot, slod_lod_factor **out)
  {
    hipStream_t st;
    if (const int rc = slod_enter(h, nullptr, &st))
      return rc;
    const SlodGrid G = slod_grid_of(h);
    const int      s = G.spacedim, w = 2 * G.oversampling + 1, cap = slod_lod_row_capacity(h);
    slod_lod_factor f;
    f.h         = h;
    f.kind      = kind;
    f.n         = h->NP * s;
    f.b         = s * (w * G.N + w) + s - 1;
    f.nb        = (f.n + FB - 1) / FB;
    f.bb        = (f.b + FB - 1) / FB;
    f.n_members = n_members;
    // one allocation: per member the band, the factored diagonal tiles, the pivots and the reciprocal diagonal of L, then
    // the row map and the status words
    const bool   ldl = kind == SLOD_FACTOR_LDL;
    const size_t npad = (size_t)f.nb * FB, nband = (size_t)f.nb * (f.bb + 1) * FT, nread = npad + (ldl ? 2 : 0);
    const size_t nd = nband + (size_t)f.nb * FT + nread + npad + (ldl ? 2 * npad : 0);
    const size_t K    = (size_t)n_members;
    f.member_doubles  = nd;
    f.bytes           = K * nd * sizeof(double) + (npad + K) * sizeof(int);
    hipError_t e      = f.mem.alloc(f.bytes); // freed with f on every error return below
    if (e != hipSuccess)
      return slod_hip_fail(h, e, who);
    f.band   = (double *)f.mem.get();
    f.diag   = f.band + nband;
    f.piv    = f.diag + (size_t)f.nb * FT;
    f.dinv   = f.piv + nread;
    f.rowmap = (int *)(f.band + K * nd);
    f.status = f.rowmap + npad;
    std::vector<double> piv(K * nread);
    std::vector<int>    bad(K, -1);
    e = hipMemsetAsync(f.band, 0, K * nd * sizeof(double), st);
    if (e == hipSuccess)
      e = hipMemsetAsync(f.status, 0xff, K * sizeof(int), st); // -1
    if (e == hipSuccess)
      {
        const size_t nval = (size_t)h->NP * cap * s * s;
        hipLaunchKernelGGL(k_factor_rowmap, dim3((unsigned)((npad + 255) / 256), (unsigned)K), dim3(256), 0, st, G, f.n, (int)npad, f.bb,
                           f.rowmap, f.band, nd);
        hipLaunchKernelGGL(k_factor_scatter, dim3((unsigned)((nval * K + 255) / 256)), dim3(256), 0, st, G, h->NP, cap, f.bb, n_members,
                           d_values, ld_m, d_cols, f.band, nd);
        // LDL^T only: the two norms behind a member's pivots, two vectors of row sums behind its dinv
        double    *norms = f.piv + npad, *work = f.dinv + npad, *work2 = work + npad;
        const dim3 rows_grid((unsigned)f.nb, (unsigned)K);
        if (ldl)
          {
            hipLaunchKernelGGL(k_ldl_norms<0>, rows_grid, dim3(256), 0, st, f.nb, f.bb, f.band, f.diag, f.piv, nullptr, work, nd);
            hipLaunchKernelGGL(k_ldl_norm_max, dim3(1, (unsigned)K), dim3(256), 0, st, f.n, work, norms, nd);
          }
        for (int col = 0; col < f.nb; ++col)
          {
            const dim3 grid((unsigned)(std::min(f.bb, f.nb - 1 - col) + 1), (unsigned)K);
            if (ldl)
              hipLaunchKernelGGL(k_ldl_column, grid, dim3(64), 0, st, col, f.bb, f.band, f.diag, f.piv, f.dinv, f.status, nd);
            else
              hipLaunchKernelGGL(k_factor_column, grid, dim3(64), 0, st, col, f.bb, f.band, f.diag, f.piv, f.dinv, f.status, nd);
          }
        if (ldl) // (a member that failed has not finished its factor: its second norm is not used)
          {
            hipLaunchKernelGGL(k_ldl_norms<1>, rows_grid, dim3(256), 0, st, f.nb, f.bb, f.band, f.diag, f.piv, nullptr, work, nd);
            hipLaunchKernelGGL(k_ldl_norms<2>, rows_grid, dim3(256), 0, st, f.nb, f.bb, f.band, f.diag, f.piv, work, work2, nd);
            hipLaunchKernelGGL(k_ldl_norm_max, dim3(1, (unsigned)K), dim3(256), 0, st, f.n, work2, norms + 1, nd);
          }
        e = hipGetLastError();
      }
    // one read-back: the pivots of every member (npad doubles every nd; behind them the two norms of an LDL^T factor) and
    // the status words
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(piv.data(), nread * sizeof(double), f.piv, nd * sizeof(double), nread * sizeof(double), K,
                           hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(bad.data(), f.status, K * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
      e = hipStreamSynchronize(st);
    if (e != hipSuccess)
      {
        (void)hipStreamSynchronize(st); // nothing may still run on the band when f frees it
        return slod_hip_fail(h, e, who);
      }
    if (bad_pivot)
      std::copy(bad.begin(), bad.end(), bad_pivot);
    for (size_t k = 0; k < K; ++k)
      if (bad[k] >= 0)
        {
          char        msg[200], member[40] = "";
          const char *what = ldl ? "is zero or not finite" : "is not positive";
          const char *why  = ldl ? "" : ": the matrix is not positive definite";
          if (ensemble)
            std::snprintf(member, sizeof member, "member %zu: ", k);
          std::snprintf(msg, sizeof msg, "%s: %spivot %d of %d %s (%g)%s", who, member, bad[k], f.n, what, piv[k * nread + (size_t)bad[k]],
                        why);
          return slod_fail(h, SLOD_ERR_NUMERIC, msg);
        }
    f.member_min.resize(K), f.member_max.resize(K);
    if (ldl)
      f.inertia.resize(K);
    for (size_t k = 0; k < K; ++k)
      {
        const double *d = piv.data() + k * nread;
        f.member_min[k] = *std::min_element(d, d + f.n);
        f.member_max[k] = *std::max_element(d, d + f.n);
        if (!ldl)
          continue;
        slod_lod_factor_inertia_host &in = f.inertia[k];
        in.min_abs = in.max_abs = std::fabs(d[0]);
        for (int r = 0; r < f.n; ++r)
          {
            (d[r] < 0.0 ? in.n_negative : in.n_positive) += 1;
            in.min_abs = std::min(in.min_abs, std::fabs(d[r]));
            in.max_abs = std::max(in.max_abs, std::fabs(d[r]));
          }
        in.norm_matrix = d[npad];
        in.norm_factor = d[npad + 1];
      }
    f.min_pivot = *std::min_element(f.member_min.begin(), f.member_min.end());
    f.max_pivot = *std::max_element(f.member_max.begin(), f.member_max.end());
    *out        = new slod_lod_factor(std::move(f));
    return SLOD_OK;
  }
} // namespace

// The complex factor: one allocation, per member  band (re, im), diagonal tiles (re, im), D (re, im), the two norms,
// 1 / D (re, im), two vectors of row sums;  then the coefficients of all members, the row map and the status words.
// d_c given: the third term gamma_k C of slod_lod_factor_create_zldl3, its coefficients behind those of the two.
int slod_lod_zfactor_launch(slod_handle *h, hipStream_t st, const char *who, const double *d_a, size_t ld_a, const double *d_b,
                            size_t ld_b, int kmat, const uint32_t *d_cols, const double *alpha, const double *beta, size_t j0,
                            int n_members, SlodZFactorBuild *z, const double *d_c, size_t ld_c, const double *gamma)
{
  const SlodGrid   G = slod_grid_of(h);
  const int        s = G.spacedim, w = 2 * G.oversampling + 1, cap = slod_lod_row_capacity(h);
  slod_lod_factor &f = z->f;
  f.h         = h;
  f.kind      = SLOD_FACTOR_ZLDL;
  f.n         = h->NP * s;
  f.b         = s * (w * G.N + w) + s - 1;
  f.nb        = (f.n + FB - 1) / FB;
  f.bb        = (f.b + FB - 1) / FB;
  f.n_members = n_members;
  const size_t npad = (size_t)f.nb * FB, nband = (size_t)f.nb * (f.bb + 1) * FT, ndiag = (size_t)f.nb * FT, nread = 2 * npad + 2;
  const size_t nd = 2 * nband + 2 * ndiag + nread + 4 * npad, K = (size_t)n_members;
  f.im_band = nband, f.im_diag = ndiag, f.im_vec = npad;
  f.member_doubles = nd;
  const size_t ncoef = d_c ? 6 : 4; // per member: alpha, beta and, with a third term, gamma
  f.bytes          = (K * nd + ncoef * K) * sizeof(double) + (npad + K) * sizeof(int);
  hipError_t e     = f.mem.alloc(f.bytes); // freed with z on every error return
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who);
  f.band   = (double *)f.mem.get();
  f.diag   = f.band + 2 * nband;
  f.piv    = f.diag + 2 * ndiag;
  f.dinv   = f.piv + nread;
  f.coef   = f.band + K * nd;
  f.rowmap = (int *)(f.coef + ncoef * K);
  f.status = f.rowmap + npad;
  z->piv.assign(K * nread, 0.0);
  z->bad.assign(K, -1);
  std::vector<double> &coef = z->coef; // lives until finish() has waited
  coef.resize(ncoef * K);
  for (size_t k = 0; k < K; ++k)
    {
      const size_t c = (j0 + k) / (size_t)kmat; // the coefficient pair of flat member j0 + k
      coef[4 * k] = alpha[2 * c], coef[4 * k + 1] = alpha[2 * c + 1], coef[4 * k + 2] = beta[2 * c], coef[4 * k + 3] = beta[2 * c + 1];
      if (d_c)
        coef[4 * K + 2 * k] = gamma[2 * c], coef[4 * K + 2 * k + 1] = gamma[2 * c + 1];
    }
  e = hipMemsetAsync(f.band, 0, K * nd * sizeof(double), st);
  if (e == hipSuccess)
    e = hipMemsetAsync(f.status, 0xff, K * sizeof(int), st); // -1
  if (e == hipSuccess)
    e = hipMemcpyAsync(f.coef, coef.data(), ncoef * K * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    {
      const size_t nval = (size_t)h->NP * cap * s * s;
      hipLaunchKernelGGL(k_factor_rowmap, dim3((unsigned)((npad + 255) / 256), (unsigned)K), dim3(256), 0, st, G, f.n, (int)npad, f.bb,
                         f.rowmap, f.band, nd);
      hipLaunchKernelGGL(d_c ? k_zfactor_scatter<true> : k_zfactor_scatter<false>, dim3((unsigned)((nval * K + 255) / 256)), dim3(256), 0,
                         st, G, h->NP, cap, f.bb, n_members, d_a, ld_a, d_b, ld_b, d_c, ld_c, kmat, j0, f.coef, f.coef + 4 * K, d_cols,
                         f.band, nband, nd);
      double    *norms = f.piv + 2 * npad, *work = f.dinv + 2 * npad, *work2 = work + npad;
      const dim3 rows_grid((unsigned)f.nb, (unsigned)K);
      hipLaunchKernelGGL(k_zldl_norms<0>, rows_grid, dim3(256), 0, st, f.nb, f.bb, f.band, nband, f.diag, ndiag, f.piv, npad, nullptr,
                         work, nd);
      hipLaunchKernelGGL(k_ldl_norm_max, dim3(1, (unsigned)K), dim3(256), 0, st, f.n, work, norms, nd);
      for (int col = 0; col < f.nb; ++col)
        {
          const dim3 grid((unsigned)(std::min(f.bb, f.nb - 1 - col) + 1), (unsigned)K);
          hipLaunchKernelGGL(k_zldl_column, grid, dim3(64), 0, st, col, f.bb, f.band, nband, f.diag, ndiag, f.piv, f.dinv, npad,
                             f.status, nd);
        }
      // (a member that failed has not finished its factor: its second norm is not used)
      hipLaunchKernelGGL(k_zldl_norms<1>, rows_grid, dim3(256), 0, st, f.nb, f.bb, f.band, nband, f.diag, ndiag, f.piv, npad, nullptr,
                         work, nd);
      hipLaunchKernelGGL(k_zldl_norms<2>, rows_grid, dim3(256), 0, st, f.nb, f.bb, f.band, nband, f.diag, ndiag, f.piv, npad, work,
                         work2, nd);
      hipLaunchKernelGGL(k_ldl_norm_max, dim3(1, (unsigned)K), dim3(256), 0, st, f.n, work2, norms + 1, nd);
      e = hipGetLastError();
    }
  if (e != hipSuccess)
    {
      (void)hipStreamSynchronize(st); // nothing may still run on the band when z frees it
      return slod_hip_fail(h, e, who);
    }
  return SLOD_OK;
}

int slod_lod_zfactor_finish(slod_handle *h, hipStream_t st, const char *who, const char *what, size_t first, SlodZFactorBuild *z,
                            int32_t *bad_pivot, const char *what_minor, int kmat)
{
  slod_lod_factor &f = z->f;
  const size_t     npad = (size_t)f.nb * FB, nread = 2 * npad + 2, nd = f.member_doubles, K = (size_t)f.n_members;
  // one read-back: D of every member (two planes, behind them the two norms) and the status words
  hipError_t e = hipMemcpy2DAsync(z->piv.data(), nread * sizeof(double), f.piv, nd * sizeof(double), nread * sizeof(double), K,
                                  hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(z->bad.data(), f.status, K * sizeof(int), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st); // on every path: nothing may still run on the band when z frees it
  if (e == hipSuccess)
    e = es;
  if (e != hipSuccess)
    return slod_hip_fail(h, e, who);
  if (bad_pivot)
    std::copy(z->bad.begin(), z->bad.end(), bad_pivot);
  for (size_t k = 0; k < K; ++k)
    if (z->bad[k] >= 0)
      {
        char          msg[240];
        const double *d = z->piv.data() + k * nread + (size_t)z->bad[k];
        if (what_minor)
          std::snprintf(msg, sizeof msg, "%s: %s %zu, %s %zu: pivot %d of %d is zero or not finite (%g, %g)", who, what,
                        (first + k) / (size_t)kmat, what_minor, (first + k) % (size_t)kmat, z->bad[k], f.n, d[0], d[npad]);
        else
          std::snprintf(msg, sizeof msg, "%s: %s %zu: pivot %d of %d is zero or not finite (%g, %g)", who, what, first + k,
                        z->bad[k], f.n, d[0], d[npad]);
        return slod_fail(h, SLOD_ERR_NUMERIC, msg);
      }
  f.member_min.resize(K), f.member_max.resize(K), f.inertia.resize(K);
  for (size_t k = 0; k < K; ++k)
    {
      const double                 *d = z->piv.data() + k * nread;
      slod_lod_factor_inertia_host &in = f.inertia[k];
      in.n_negative = in.n_positive = -1; // a complex D has no signs
      in.min_abs = in.max_abs = std::hypot(d[0], d[npad]);
      for (int r = 1; r < f.n; ++r)
        {
          const double a = std::hypot(d[r], d[npad + r]);
          in.min_abs     = std::min(in.min_abs, a);
          in.max_abs     = std::max(in.max_abs, a);
        }
      in.norm_matrix  = d[2 * npad];
      in.norm_factor  = d[2 * npad + 1];
      f.member_min[k] = in.min_abs;
      f.member_max[k] = in.max_abs;
    }
  f.min_pivot = *std::min_element(f.member_min.begin(), f.member_min.end());
  f.max_pivot = *std::max_element(f.member_max.begin(), f.member_max.end());
  return SLOD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int slod_lod_factor_create(slod_handle *h, const double *d_values, const uint32_t *d_cols, slod_lod_factor **out)
{
  if (out)
    *out = nullptr;
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_values || !d_cols || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_factor_create: NULL array or out");
  return factor_create(h, "slod_lod_factor_create", false, SLOD_FACTOR_CHOLESKY, d_values, 1, 1, d_cols, nullptr, out);
}

int slod_lod_factor_create_ldl(slod_handle *h, const double *d_values, const uint32_t *d_cols, slod_lod_factor **out)
{
  if (out)
    *out = nullptr;
  if (!h)
    return SLOD_ERR_ARGUMENT;
  if (!d_values || !d_cols || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_factor_create_ldl: NULL array or out");
  return factor_create(h, "slod_lod_factor_create_ldl", false, SLOD_FACTOR_LDL, d_values, 1, 1, d_cols, nullptr, out);
}

// the body of the two ensemble create calls: their argument checks, then factor_create
static int factor_create_ensemble(const char *who, int kind, slod_handle *h, const double *d_values, size_t ld_m, int n_members,
                                  const uint32_t *d_cols, int32_t *bad_pivot, slod_lod_factor **out)
{
  if (out)
    *out = nullptr;
  if (!h || !d_values || !d_cols || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle, array or out");
  if (n_members < 1 || n_members > MAX_MEMBERS)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or > 65535");
  if (const int rc = slod_check_ld(h, who, "n_members", n_members, {ld_m}))
    return rc;
  return factor_create(h, who, true, kind, d_values, ld_m, n_members, d_cols, bad_pivot, out);
}

int slod_lod_factor_create_ensemble(slod_handle *h, const double *d_values, size_t ld_m, int n_members, const uint32_t *d_cols,
                                    int32_t *bad_pivot, slod_lod_factor **out)
{
  return factor_create_ensemble("slod_lod_factor_create_ensemble", SLOD_FACTOR_CHOLESKY, h, d_values, ld_m, n_members, d_cols, bad_pivot,
                                out);
}

int slod_lod_factor_create_ldl_ensemble(slod_handle *h, const double *d_values, size_t ld_m, int n_members, const uint32_t *d_cols,
                                        int32_t *bad_pivot, slod_lod_factor **out)
{
  return factor_create_ensemble("slod_lod_factor_create_ldl_ensemble", SLOD_FACTOR_LDL, h, d_values, ld_m, n_members, d_cols, bad_pivot,
                                out);
}

int slod_lod_factor_inertia(const slod_lod_factor *f, int member, slod_lod_factor_inertia_info *out)
{
  const char *who = "slod_lod_factor_inertia";
  if (!f || !out)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL factor or out"); // (the factor is not read)
  if (member < 0 || member >= f->n_members)
    return slod_fail(f->h, SLOD_ERR_ARGUMENT, std::string(who) + ": no such member");
  if (f->kind == SLOD_FACTOR_CHOLESKY)
    return slod_fail(f->h, SLOD_ERR_ARGUMENT, std::string(who) + ": a Cholesky factor has no inertia to report; use slod_lod_factor_create_ldl");
  const slod_lod_factor_inertia_host &in = f->inertia[(size_t)member];
  out->n_negative    = in.n_negative;
  out->n_positive    = in.n_positive;
  out->min_abs_pivot = in.min_abs;
  out->max_abs_pivot = in.max_abs;
  out->norm_matrix   = in.norm_matrix;
  out->norm_factor   = in.norm_factor;
  return SLOD_OK;
}

int slod_lod_factor_get_info(const slod_lod_factor *f, slod_lod_factor_info *info)
{
  if (!f || !info)
    return SLOD_ERR_ARGUMENT;
  info->n              = f->n;
  info->half_bandwidth = f->b;
  info->block          = FB;
  info->bytes          = f->bytes;
  info->min_pivot      = f->min_pivot;
  info->max_pivot      = f->max_pivot;
  return SLOD_OK;
}

int slod_lod_factor_get_info_member(const slod_lod_factor *f, int member, slod_lod_factor_info *info)
{
  if (!f || !info)
    return slod_fail(f ? f->h : nullptr, SLOD_ERR_ARGUMENT, "slod_lod_factor_get_info_member: NULL factor or info");
  if (member < 0 || member >= f->n_members)
    return slod_fail(f->h, SLOD_ERR_ARGUMENT, "slod_lod_factor_get_info_member: no such member");
  slod_lod_factor_get_info(f, info);
  info->min_pivot = f->member_min[(size_t)member];
  info->max_pivot = f->member_max[(size_t)member];
  return SLOD_OK;
}

int slod_lod_factor_solve(slod_lod_factor *f, const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u, size_t ld_u, void *hip_stream)
{
  if (!f)
    return SLOD_ERR_ARGUMENT;
  slod_handle *h = f->h;
  if (!d_rhs || !d_u)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_factor_solve: NULL array");
  if (n_rhs < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_factor_solve: n_rhs < 1");
  if (const int rc = slod_check_ld(h, "slod_lod_factor_solve", "n_rhs", n_rhs, {ld_rhs, ld_u}))
    return rc;
  if (f->kind == SLOD_FACTOR_ZLDL)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string("slod_lod_factor_solve") + COMPLEX_REFUSED);
  if (f->n_members != 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, "slod_lod_factor_solve: an ensemble factor of several members; use slod_lod_factor_solve_ensemble");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  slod_lod_factor_solve_launch(f, st, d_rhs, ld_rhs, n_rhs, d_u, ld_u);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, "slod_lod_factor_solve");
}

int slod_lod_factor_solve_ensemble(slod_lod_factor *f, int first_member, int n_members, const double *d_rhs, size_t ld_rhs, int n_rhs,
                                   double *d_u, size_t ld_u, void *hip_stream)
{
  const char *who = "slod_lod_factor_solve_ensemble";
  if (!f)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL factor");
  slod_handle *h = f->h;
  if (!d_rhs || !d_u)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL array");
  if (n_rhs < 1 || n_members < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_rhs < 1 or n_members < 1");
  if (f->kind == SLOD_FACTOR_ZLDL)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + COMPLEX_REFUSED);
  if (first_member < 0 || first_member > f->n_members - n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": members outside the factor");
  for (const size_t ld : {ld_rhs, ld_u})
    if (ld / (size_t)n_rhs < (size_t)n_members)
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": leading dimension below n_members * n_rhs");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  slod_lod_factor_solve_launch(f, st, d_rhs, ld_rhs, n_rhs, d_u, ld_u, first_member, n_members);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_factor_create_zldl(slod_handle *h, const double *d_a, const double *d_b, const uint32_t *d_cols, const double *alpha,
                                const double *beta, int n_members, int32_t *bad_pivot, slod_lod_factor **out)
{
  const char *who = "slod_lod_factor_create_zldl";
  if (out)
    *out = nullptr;
  if (!h || !d_a || !d_b || !d_cols || !alpha || !beta || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle, array, alpha, beta or out");
  if (n_members < 1 || n_members > MAX_MEMBERS)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or > 65535");
  for (int k = 0; k < 2 * n_members; ++k)
    if (!std::isfinite(alpha[k]) || !std::isfinite(beta[k]))
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": a coefficient is NaN or infinite");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  SlodZFactorBuild z;
  if (const int rc = slod_lod_zfactor_launch(h, st, who, d_a, 1, d_b, 1, 1, d_cols, alpha, beta, 0, n_members, &z))
    return rc;
  if (const int rc = slod_lod_zfactor_finish(h, st, who, "member", 0, &z, bad_pivot))
    return rc;
  *out = new slod_lod_factor(std::move(z.f));
  return SLOD_OK;
}

// slod_lod_factor_create_zldl with a third term:  S_k = alpha_k A + beta_k B + gamma_k C
int slod_lod_factor_create_zldl3(slod_handle *h, const double *d_a, const double *d_b, const double *d_c, const uint32_t *d_cols,
                                 const double *alpha, const double *beta, const double *gamma, int n_members, int32_t *bad_pivot,
                                 slod_lod_factor **out)
{
  const char *who = "slod_lod_factor_create_zldl3";
  if (out)
    *out = nullptr;
  if (!h || !d_a || !d_b || !d_c || !d_cols || !alpha || !beta || !gamma || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle, array, alpha, beta, gamma or out");
  if (n_members < 1 || n_members > MAX_MEMBERS)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or > 65535");
  for (int k = 0; k < 2 * n_members; ++k)
    if (!std::isfinite(alpha[k]) || !std::isfinite(beta[k]) || !std::isfinite(gamma[k]))
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": a coefficient is NaN or infinite");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  SlodZFactorBuild z;
  if (const int rc = slod_lod_zfactor_launch(h, st, who, d_a, 1, d_b, 1, 1, d_cols, alpha, beta, 0, n_members, &z, d_c, 1, gamma))
    return rc;
  if (const int rc = slod_lod_zfactor_finish(h, st, who, "member", 0, &z, bad_pivot))
    return rc;
  *out = new slod_lod_factor(std::move(z.f));
  return SLOD_OK;
}

int slod_lod_factor_create_zldl_ensemble(slod_handle *h, const double *d_a, size_t ld_a_m, const double *d_b, size_t ld_b_m,
                                         int n_members, const uint32_t *d_cols, const double *alpha, const double *beta, int n_coef,
                                         int32_t *bad_pivot, slod_lod_factor **out)
{
  const char *who = "slod_lod_factor_create_zldl_ensemble";
  if (out)
    *out = nullptr;
  if (!h || !d_a || !d_b || !d_cols || !alpha || !beta || !out)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL handle, array, alpha, beta or out");
  if (n_members < 1 || n_members > MAX_MEMBERS)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_members < 1 or > 65535");
  if (n_coef < 1 || n_coef > MAX_MEMBERS / n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_coef < 1 or n_coef * n_members > 65535");
  if (ld_a_m < (size_t)n_members || ld_b_m < (size_t)n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": leading dimension of a matrix below n_members");
  for (int k = 0; k < 2 * n_coef; ++k)
    if (!std::isfinite(alpha[k]) || !std::isfinite(beta[k]))
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": a coefficient is NaN or infinite");
  hipStream_t st;
  if (const int rc = slod_enter(h, nullptr, &st))
    return rc;
  SlodZFactorBuild z;
  if (const int rc = slod_lod_zfactor_launch(h, st, who, d_a, ld_a_m, d_b, ld_b_m, n_members, d_cols, alpha, beta, 0,
                                             n_coef * n_members, &z))
    return rc;
  if (const int rc = slod_lod_zfactor_finish(h, st, who, "coefficient", 0, &z, bad_pivot, "member", n_members))
    return rc;
  *out = new slod_lod_factor(std::move(z.f));
  return SLOD_OK;
}

int slod_lod_factor_solve_complex(slod_lod_factor *f, int first_member, int n_members, const double *d_rhs_re, const double *d_rhs_im,
                                  size_t ld_rhs, int n_rhs, int shared_rhs, double *d_u_re, double *d_u_im, size_t ld_u,
                                  void *hip_stream)
{
  const char *who = "slod_lod_factor_solve_complex";
  if (!f)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL factor");
  slod_handle *h = f->h;
  if (!d_rhs_re || !d_u_re || !d_u_im)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL array");
  if (n_rhs < 1 || n_members < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_rhs < 1 or n_members < 1");
  if (f->kind != SLOD_FACTOR_ZLDL)
    return slod_fail(h, SLOD_ERR_ARGUMENT,
                     std::string(who) + ": a real factor (slod_lod_factor_create, _create_ldl) is solved by slod_lod_factor_solve");
  if (first_member < 0 || first_member > f->n_members - n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": members outside the factor");
  if (ld_u / (size_t)n_rhs < (size_t)n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": leading dimension of u below n_members * n_rhs");
  if (shared_rhs ? ld_rhs < (size_t)n_rhs : ld_rhs / (size_t)n_rhs < (size_t)n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT,
                     std::string(who) + (shared_rhs ? ": leading dimension of the shared rhs below n_rhs"
                                                    : ": leading dimension of the rhs below n_members * n_rhs"));
  if (shared_rhs && n_members > 1)
    for (const double *u : {d_u_re, d_u_im})
      if (u == d_rhs_re || u == d_rhs_im)
        return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": a shared rhs of several members cannot be solved in place");
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  slod_lod_zfactor_solve_launch(f, st, first_member, n_members, d_rhs_re, d_rhs_im, ld_rhs, n_rhs, 0, shared_rhs ? 1 : n_members,
                                d_u_re, d_u_im, ld_u);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

int slod_lod_factor_solve_complex_ensemble(slod_lod_factor *f, int first_member, int n_members, const double *d_rhs_re,
                                           const double *d_rhs_im, size_t ld_rhs, int n_rhs, int rhs_members, double *d_u_re,
                                           double *d_u_im, size_t ld_u, void *hip_stream)
{
  const char *who = "slod_lod_factor_solve_complex_ensemble";
  if (!f)
    return slod_fail(nullptr, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL factor");
  slod_handle *h = f->h;
  if (!d_rhs_re || !d_u_re || !d_u_im)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": NULL array");
  if (n_rhs < 1 || n_members < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": n_rhs < 1 or n_members < 1");
  if (rhs_members < 1)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": rhs_members < 1");
  if (f->kind != SLOD_FACTOR_ZLDL)
    return slod_fail(h, SLOD_ERR_ARGUMENT,
                     std::string(who) + ": a real factor (slod_lod_factor_create, _create_ldl) is solved by slod_lod_factor_solve");
  if (first_member < 0 || first_member > f->n_members - n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": members outside the factor");
  if (ld_u / (size_t)n_rhs < (size_t)n_members)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": leading dimension of u below n_members * n_rhs");
  // the rhs columns read: those of the members j % rhs_members, j = first_member .. first_member + n_members - 1
  const int rhs_first = first_member % rhs_members;
  const int rhs_used  = n_members >= rhs_members || rhs_first + n_members > rhs_members ? rhs_members : rhs_first + n_members;
  if (ld_rhs / (size_t)n_rhs < (size_t)rhs_used)
    return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": leading dimension of the rhs below the columns read");
  // in place only where every member reads the columns it writes: j % rhs_members = j - first_member for all of them
  if (n_members > rhs_members || rhs_first != 0)
    for (const double *u : {d_u_re, d_u_im})
      if (u == d_rhs_re || u == d_rhs_im)
        return slod_fail(h, SLOD_ERR_ARGUMENT,
                         std::string(who) + (n_members > rhs_members
                                               ? ": rhs columns read by several members cannot be solved in place"
                                               : ": in place needs first_member to be a multiple of rhs_members"));
  hipStream_t st;
  if (const int rc = slod_enter(h, hip_stream, &st))
    return rc;
  slod_lod_zfactor_solve_launch(f, st, first_member, n_members, d_rhs_re, d_rhs_im, ld_rhs, n_rhs, rhs_first, rhs_members, d_u_re,
                                d_u_im, ld_u);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who);
}

void slod_lod_factor_destroy(slod_lod_factor *f)
{
  if (!f)
    return;
  (void)hipSetDevice(f->h->cfg.device);
  (void)hipStreamSynchronize(f->h->stream); // a solve on the handle's stream may still read the band
  delete f;
}

} // extern "C"
#pragma GCC visibility pop
