// Host-side internals of libslod_hip.so shared by slod_api.cpp and the .hip units of the global steps
// (not part of the public ABI).
#ifndef SLOD_HOST_H
#define SLOD_HOST_H
#pragma GCC visibility push(default)
#include "../../include/slod.h"
#pragma GCC visibility pop
#include "slod_device.h"

#include <algorithm>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

struct slod_handle
{
  slod_config         cfg;
  int                 N  = 0; // coarse cells per side
  int                 NE = 0; // fine elements per side
  int                 NP = 0; // patches per problem
  int                 first_full = -1;
  double             *d_coef[2]  = {nullptr, nullptr};
  std::vector<char>   coef_set;  // [problem*2 + field]
  hipStream_t         stream = nullptr;
  bool                device_ready = false; // stream and coefficient storage exist
  double             *d_err_ws = nullptr;   // slod_compute_error_norms partials (slod_error.hip), on first use
  slod_lod_time_record record{};            // slod_lod_time_record_arm: what the next stepper call takes off the handle
  bool                record_armed = false;
  slod_lod_time_source source{};            // slod_lod_time_source_arm: what drives the next stepper call, taken with the record
  bool                source_armed = false;
  mutable std::string error;
};

// error text of the last failed slod_create on this thread (slod_api.cpp)
std::string &slod_create_error();
inline int   slod_fail(const slod_handle *h, int code, const std::string &msg)
{
  if (h)
    h->error = msg;
  else
    slod_create_error() = msg;
  return code;
}
inline int slod_hip_fail(const slod_handle *h, hipError_t e, const char *what)
{
  return slod_fail(h, SLOD_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
// stream + coefficient storage; called by every entry point that touches the device (slod_api.cpp)
int slod_ensure_device(slod_handle *h);
// The prologue of an entry point once its argument checks have passed: the device exists and is current,
// *st (st may be null) is the caller's stream or, for a null hip_stream, the handle's.  0 or the status to return.
inline int slod_enter(slod_handle *h, void *hip_stream, hipStream_t *st)
{
  if (const int rc = slod_ensure_device(h))
    return rc;
  (void)hipSetDevice(h->cfg.device);
  if (st)
    *st = hip_stream ? (hipStream_t)hip_stream : h->stream;
  return SLOD_OK;
}
// Move-only owner of one hipMalloc, freed when it leaves scope: the stream that used the memory must have
// been synchronised by then.
template <typename T>
class SlodDevBuf
{
public:
  SlodDevBuf() = default;
  SlodDevBuf(SlodDevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
  ~SlodDevBuf() { if (p) (void)hipFree(p); }
  // count objects of T, uninitialised; once per owner
  hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
  T         *get() const { return p; }

private:
  T *p = nullptr;
};
// A caller-owned host array of row patch ids.  slod_check_rows: an id that is no patch of the handle is
// SLOD_ERR_ARGUMENT, "<who>: row patch id out of range" (who NULL: no prefix).  slod_upload_rows: that check,
// then the copy to d_rows, synchronised on st.
inline int slod_check_rows(const slod_handle *h, const char *who, const uint32_t *rows, size_t n)
{
  for (size_t k = 0; k < n; ++k)
    if (rows[k] >= (uint32_t)h->NP)
      return slod_fail(h, SLOD_ERR_ARGUMENT, (who ? std::string(who) + ": " : std::string()) + "row patch id out of range");
  return SLOD_OK;
}
inline int slod_upload_rows(slod_handle *h, const char *who, const uint32_t *rows, size_t n, hipStream_t st,
                            SlodDevBuf<uint32_t> *d_rows)
{
  if (const int rc = slod_check_rows(h, who, rows, n))
    return rc;
  hipError_t e = d_rows->alloc(std::max<size_t>(n, 1));
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_rows->get(), rows, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); // rows is a caller-owned host array
  return e == hipSuccess ? SLOD_OK : slod_hip_fail(h, e, who ? who : "row upload");
}
// Device copy of the index calculus a kernel needs: everything derives from these scalars.
struct SlodGrid
{
  int32_t N, n_sub, oversampling, spacedim, morton_bits; // morton_bits < 0: row-major patch ids
  int32_t lod_stabilization;
};
inline SlodGrid slod_grid_of(const slod_handle *h)
{
  SlodGrid g;
  g.N                 = h->N;
  g.n_sub             = h->cfg.n_subdivisions;
  g.oversampling      = h->cfg.oversampling;
  g.spacedim          = h->cfg.spacedim;
  g.morton_bits       = h->cfg.n_cells_per_side > 0 ? -1 : h->cfg.n_global_refinements;
  g.lod_stabilization = h->cfg.lod_stabilization;
  return g;
}
// doubles per patch of a uniform-stride slab (slod_plan_stride()): the full patch's s vectors of n_fine
inline size_t slod_uniform_stride(const slod_handle *h)
{
  const size_t s = (size_t)h->cfg.spacedim, side = (size_t)h->cfg.n_subdivisions * (2 * (size_t)h->cfg.oversampling + 1) + 1;
  return s * s * side * side;
}
// plan construction on the device (slod_plan_build.hip: k_make_desc, k_balance_order)
struct SlodPlanSummary
{
  int32_t            m_max, L_max, nc_max, nb_max, nn_max, error;
  unsigned long long out_size;
};
struct SlodPlanBuild
{
  const uint32_t  *gids;
  const uint64_t  *offsets; // may be null: uniform stride
  size_t           n, stride;
  int32_t          NP, n_problems, reuse_full, first_full;
  SlodPatchDesc   *desc;
  double          *cost;
  SlodPlanSummary *acc;
  char            *prob_used;
};
hipError_t slod_build_descriptors(const slod_handle *h, const uint32_t *gids, size_t n, const uint64_t *offsets, size_t stride,
                                  int n_cu, bool balance, SlodPatchDesc *d_desc, SlodPatchDesc *d_desc_bal, SlodPlanSummary *sum,
                                  std::vector<char> *prob_used);
// ---- shared by the units of the LOD space (slod_lod_multi/time/wave/eig.hip)
// Y = A X on a full set of block rows, the launch of slod_lod_apply_multi (slod_lod_time.hip)
void slod_lod_apply_launch(const slod_handle *h, hipStream_t st, const double *d_values, const uint32_t *d_cols, const double *d_x,
                           size_t ld_x, int n_rhs, double *d_y, size_t ld_y);
// out = alpha a + beta b on n values, the launch of slod_lod_matrix_combine (slod_lod_time.hip)
void slod_lod_combine_launch(hipStream_t st, size_t n, double alpha, const double *d_a, double beta, const double *d_b, double *d_out);
// SLOD_ERR_ARGUMENT, "<who>: leading dimension below <what>", when one of lds is below n; else SLOD_OK
inline int slod_check_ld(const slod_handle *h, const char *who, const char *what, int n, std::initializer_list<size_t> lds)
{
  for (const size_t ld : lds)
    if (ld < (size_t)n)
      return slod_fail(h, SLOD_ERR_ARGUMENT, std::string(who) + ": leading dimension below " + what);
  return SLOD_OK;
}
// Hands out consecutive pieces of one array of doubles.  Without a base it only counts, so a function that names its
// pieces by take() gives the size of the array on a first run and the pointers on a second: the two cannot disagree.
struct SlodCarver
{
  double *base = nullptr;
  size_t  used = 0;
  double *take(size_t count) { used += count; return base ? base + (used - count) : nullptr; }
  template <typename T> // one object of T in a slot of its own, whole doubles
  T *take_as() { return (T *)take((sizeof(T) + sizeof(double) - 1) / sizeof(double)); }
};
// The device workspace of a call that runs the solve of slod_lod_solve_multi, once or in a loop: one array of doubles and
// the active flags of the columns, one hipMalloc each per call, freed when the owner leaves scope (the stream must have
// been synchronised by then; solve() does).
struct SlodLodWork
{
  std::vector<int>    its;                 // HOST [n_rhs], of the last solve
  std::vector<double> res;                 // HOST [n_rhs], relative residuals of the last solve
  int                 last = 0, worst = 0; // the largest its[] of the last solve, of all solves
  // carve(SlodCarver &) names every piece of the array, take_solve() among them; it runs twice, first to count
  template <typename Carve>
  hipError_t alloc(int n_rhs, Carve &&carve)
  {
    its.assign((size_t)n_rhs, 0);
    res.assign((size_t)n_rhs, 0.0);
    SlodCarver count, hand;
    carve(count);
    hipError_t e = work.alloc(count.used);
    if (e == hipSuccess)
      e = active.alloc((size_t)n_rhs);
    if (e != hipSuccess)
      return e;
    hand.base = work.get();
    carve(hand);
    return hipSuccess;
  }
  // the pieces of the solve, placed where the caller's carve calls it (slod_lod_multi.hip).  matrix_per_column: for
  // solves on an ensemble matrix (include/slod.h), which need D^-1 per column: nrow * n_rhs doubles more.
  void take_solve(SlodCarver &c, const slod_handle *h, bool matrix_per_column = false);
  // A U = RHS for the n_rhs columns, every one from zero (slod_lod_multi.hip).  Arguments are checked by the caller; the
  // handle's device is current.  Synchronises h->stream.  After take_solve(.., true) d_values is an ensemble matrix with
  // leading dimension ld_m and column k is solved with matrix k; else ld_m is not used.
  hipError_t solve(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_rhs, size_t ld_rhs, double *d_u,
                   size_t ld_u, double rel_tol, int max_iterations, size_t ld_m = 1);
  // The same for CG preconditioned by a banded factor (slod_lod_pcg.hip): take_precond() places the pieces of that
  // recurrence, solve_precond() runs it with  z = P^-1 r  by the sweeps of f, on its one member for every column or, when f
  // has several, with column k on member k.  matrix_per_column: d_values is an ensemble matrix, column k reads matrix k.
  // Synchronises h->stream on every path.  The stop rule and the counters run on the device; its, res, last and worst are
  // filled as by solve().  A column whose p.Ap is not > 0 or whose r.r is not finite freezes and the others finish: the
  // lowest such column is bad_col (-1: none), with the iteration it met it in, which of the two it was, and the value.
  void       take_precond(SlodCarver &c, const slod_handle *h);
  hipError_t solve_precond(slod_handle *h, const slod_lod_factor *f, const double *d_values, const uint32_t *d_cols,
                           const double *d_rhs, size_t ld_rhs, double *d_u, size_t ld_u, double rel_tol, int max_iterations,
                           bool matrix_per_column = false, size_t ld_m = 1);
  int        bad_col = -1, bad_it = 0;
  bool       bad_pAp = false;
  double     bad_value = 0.0;
  // what a time loop reports of step k, HOST arrays, either may be NULL: the maxima over the columns of the last solve
  void record(int k, int *iterations, double *rel_residual) const
  {
    if (iterations)
      iterations[k] = last;
    if (rel_residual)
      rel_residual[k] = *std::max_element(res.begin(), res.end());
  }
  // what a single solve reports per column, HOST [n_rhs], either may be NULL
  void report(int *iterations, double *rel_residual) const
  {
    if (iterations)
      std::copy(its.begin(), its.end(), iterations);
    if (rel_residual)
      std::copy(res.begin(), res.end(), rel_residual);
  }

private:
  SlodDevBuf<double> work;
  SlodDevBuf<int>    active;
  double            *cg = nullptr; // the pieces of the solve
  double            *pcg = nullptr; // the pieces of the preconditioned solve
  bool               per_col = false; // as given to take_solve
};
// Y_k = A_k X_k on an ensemble matrix, the launch of slod_lod_apply_ensemble (slod_lod_ensemble.hip)
void slod_lod_apply_ensemble_launch(const slod_handle *h, hipStream_t st, const double *d_values, size_t ld_m, const uint32_t *d_cols,
                                    const double *d_x, size_t ld_x, int n_members, double *d_y, size_t ld_y);
// The banded Cholesky factors of the full sets of block rows of n_members matrices on one pattern (slod_lod_factor.hip;
// a single factor has one member): 16 x 16 tiles, nb block rows, bb block sub-diagonals.  mem holds n_members copies of
// member_doubles doubles (band, factored diagonal tiles, pivots, reciprocal diagonal of L; the pointers are member 0's),
// then the row map, which all members share, and a status word per member.  kind SLOD_FACTOR_LDL: S = L D L^T without
// pivoting (k_ldl_column); the diagonal tiles hold the unit lower triangular L_II, piv is D (signed), dinv 1 / D, and a
// member has two norms behind its pivots (||S||_inf, || |L| |D| |L^T| ||_inf) and two work vectors behind dinv.
// kind SLOD_FACTOR_ZLDL: the complex symmetric S_k = alpha_k A + beta_k B = L D L^T (plain transpose, k_zldl_column) of
// slod_lod_factor_create_zldl.  Every array of a member is two planes, real then imaginary, in the layout of the real
// factor: band (im_band doubles apart), diagonal tiles (im_diag), piv = D (im_vec; the two norms follow the imaginary
// plane), dinv = 1 / D (im_vec; the two work vectors follow).  coef: (alpha_re, alpha_im, beta_re, beta_im) per member,
// behind the last member.  member_min / member_max and the inertia's pivot range are those of |D|.
enum slod_factor_kind { SLOD_FACTOR_CHOLESKY = 0, SLOD_FACTOR_LDL = 1, SLOD_FACTOR_ZLDL = 2 };
struct slod_lod_factor_inertia_host // HOST, per member of an LDL^T factor: slod_lod_factor_inertia_info of include/slod.h
{
  int    n_negative = 0, n_positive = 0;
  double min_abs = 0.0, max_abs = 0.0, norm_matrix = 0.0, norm_factor = 0.0;
};
struct slod_lod_factor
{
  slod_handle        *h = nullptr;
  int                 kind = SLOD_FACTOR_CHOLESKY;
  std::vector<slod_lod_factor_inertia_host> inertia; // HOST [n_members], LDL^T only
  int                 n = 0, b = 0, nb = 0, bb = 0; // rows, half bandwidth, block rows, block sub-diagonals
  int                 n_members = 1;
  size_t              member_doubles = 0, bytes = 0;
  double              min_pivot = 0.0, max_pivot = 0.0; // over all members
  std::vector<double> member_min, member_max;           // HOST [n_members]
  double             *band = nullptr, *diag = nullptr, *piv = nullptr, *dinv = nullptr;
  int                *rowmap = nullptr, *status = nullptr;
  size_t              im_band = 0, im_diag = 0, im_vec = 0; // SLOD_FACTOR_ZLDL: from a real plane to its imaginary one
  double             *coef = nullptr;                      // SLOD_FACTOR_ZLDL: DEVICE [n_members][4]
  SlodDevBuf<char>    mem;
};
// The parts of slod_lod_factor_create_zldl for a caller that queues more work behind the factorisation before it waits
// (slod_lod_harmonic.hip).  launch: the allocation and every kernel on st, nothing read back; alpha, beta HOST
// [(j0 + n_members - 1) / kmat + 1][2], read before it returns.  finish: after solves on the members were queued at will, the one read-back and
// wait, then the host side: bad_pivot (may be NULL), the error text "<who>: <what> <first + k>: pivot r of n is zero or
// not finite (re, im)" with SLOD_ERR_NUMERIC, or the norms and pivot ranges of every member.  Arguments are checked by
// the caller.  A failed member's band holds unfinished values: solves on it fault nothing and mean nothing.
struct SlodZFactorBuild
{
  slod_lod_factor     f;
  std::vector<double> piv, coef; // HOST: the read-back, the coefficients on their way up
  std::vector<int>    bad;
};
// d_a, d_b are ensemble matrices of kmat members (ld_a, ld_b; one matrix each: kmat = 1, ld = 1) and alpha, beta tables of
// coefficient pairs: member k of the build is the flat member j = j0 + k, with the pair j / kmat on the matrices of member
// j % kmat.  what_minor given: the error text names "<what> j / kmat, <what_minor> j % kmat", j = first + k.
// d_c given: the third term gamma_j C of slod_lod_factor_create_zldl3, d_c and gamma laid out as d_a and alpha; the device
// keeps gamma as [n_members][2] behind coef.
int slod_lod_zfactor_launch(slod_handle *h, hipStream_t st, const char *who, const double *d_a, size_t ld_a, const double *d_b,
                            size_t ld_b, int kmat, const uint32_t *d_cols, const double *alpha, const double *beta, size_t j0,
                            int n_members, SlodZFactorBuild *z, const double *d_c = nullptr, size_t ld_c = 1,
                            const double *gamma = nullptr);
int slod_lod_zfactor_finish(slod_handle *h, hipStream_t st, const char *who, const char *what, size_t first, SlodZFactorBuild *z,
                            int32_t *bad_pivot, const char *what_minor = nullptr, int kmat = 1);
// The launch of slod_lod_factor_solve_complex(_ensemble): member first_member + k reads the rhs columns
// ((rhs_first + k) % rhs_members) n_rhs .. and writes the columns k n_rhs .. of u; arguments are checked by the caller
void slod_lod_zfactor_solve_launch(const slod_lod_factor *f, hipStream_t st, int first_member, int n_members, const double *d_rhs_re,
                                   const double *d_rhs_im, size_t ld_rhs, int n_rhs, int rhs_first, int rhs_members, double *d_u_re,
                                   double *d_u_im, size_t ld_u);
// The launch of slod_lod_factor_solve_ensemble for the time loops on a factor (slod_lod_time.hip, slod_lod_wave.hip):
// member first_member + k solves the columns k n_rhs .. k n_rhs + n_rhs - 1; arguments are checked by the caller
void slod_lod_factor_solve_launch(const slod_lod_factor *f, hipStream_t st, const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u,
                                  size_t ld_u, int first_member = 0, int n_members = 1);
// out[0 .. n_rhs) = 1/2 v_c^T M v_c, out[n_rhs .. 2 n_rhs) = 1/2 u_c^T A u_c: the two launches of the energies of the Newmark
// loop (slod_lod_wave.hip) for the other time loops; d_part_k, d_part_p: ngroup * n_rhs doubles each (slod_lod_tile.hip.h).
// per_col: column c reads member c of the ensemble matrices (ld_a_m, ld_m_m), as the Newmark ensemble loop does.
void slod_lod_energies_launch(const slod_handle *h, hipStream_t st, const double *d_stiffness, const double *d_mass,
                              const uint32_t *d_cols, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                              double *d_part_k, double *d_part_p, double *d_out, bool per_col = false, size_t ld_a_m = 1,
                              size_t ld_m_m = 1);
// SLOD_ERR_ARGUMENT, "<who>: NULL factor", "<who>: factor of another handle / row count" or "<who>: factor of another
// member count" (the time loops on one matrix take a factor of one member) or "<who>: a complex factor
// (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex"; else SLOD_OK
int slod_lod_factor_check(const slod_handle *h, const char *who, const slod_lod_factor *f, int n_members = 1);
// The rows of a set of receivers over the coarse unknowns (slod_lod_receivers.hip): CSR, values member-minor
// (values[e n_members + m]); one allocation, the values first.
struct slod_lod_receivers
{
  slod_handle     *h = nullptr;
  int              n_recv = 0, n_members = 1;
  size_t           nnz = 0, bytes = 0;
  uint32_t        *row_begin = nullptr, *cols = nullptr; // DEVICE [n_recv + 1], [nnz]
  double          *values = nullptr;                     // DEVICE [nnz][n_members]
  SlodDevBuf<char> mem;
};
// The record of a time loop (slod_lod_time_record_arm).  A stepper body takes it off the handle as its first action
// (take: one-shot, whatever the call returns then), checks it after its own checks and before any device work (check: the
// refusals of include/slod.h in their order, nq = the quantities of a record), and queues one product on the loop's stream
// for the entry state and after every every-th advance (launch: record j; u and v in one launch).  Not armed: check
// returns SLOD_OK and the loop launches nothing more.
struct SlodLodRecord
{
  bool                 armed = false;
  int                  nq = 1;
  slod_lod_time_record rec{};
  // the record that the state after `steps_done` steps goes to, or -1
  int slot(int steps_done) const { return armed && steps_done % rec.every == 0 ? steps_done / rec.every : -1; }
};
SlodLodRecord slod_lod_record_take(slod_handle *h);
int  slod_lod_record_check(const slod_handle *h, const std::string &who, SlodLodRecord *r, bool has_v, int n_steps, int n, bool per_col);
void slod_lod_record_launch(hipStream_t st, const SlodLodRecord &r, int j, int n, bool per_col, const double *d_u, size_t ld_u,
                            const double *d_v, size_t ld_v);
// A set of sources (slod_lod_sources.hip): the rows of a receivers object transposed.  Coarse row r with slot[r] = t >= 0
// owns the entries begin[t] .. begin[t + 1] - 1, entry i with the source src[i] and the values values[i n_members + m],
// in the order of the receivers' entries; one allocation, the values first.
struct slod_lod_sources
{
  slod_handle     *h = nullptr;
  int              n_src = 0, n_members = 1, nrow = 0;
  uint32_t         n_touched = 0;
  size_t           nnz = 0, bytes = 0;
  double          *values = nullptr;                 // DEVICE [nnz][n_members]
  uint32_t        *begin = nullptr, *src = nullptr;  // DEVICE [n_touched + 1], [nnz]
  int32_t         *slot = nullptr;                   // DEVICE [nrow]
  SlodDevBuf<char> mem;
};
// The source of a time loop (slod_lod_time_source_arm), the mirror of the record: taken off the handle with it, checked
// after it ("<who>: source: ...", need = the samples the loop reads, bound = their count in words), and one product
// b = base + O^T g queued per step ahead of the right-hand side (launch: ny = 1 or 2 consecutive samples from `sample`, the
// base of sample y at d_base + y base_stride or NULL, written to d_b + y b_stride with the leading dimension n).
struct SlodLodSource
{
  bool                 armed = false;
  slod_lod_time_source s{};
};
SlodLodSource slod_lod_source_take(slod_handle *h);
int  slod_lod_source_check(const slod_handle *h, const std::string &who, const SlodLodSource &s, int need, const char *bound, int n,
                           bool per_col);
void slod_lod_source_launch(hipStream_t st, const SlodLodSource &s, int sample, int ny, int n, bool per_col, const double *d_base,
                            size_t ld_base, size_t base_stride, double *d_b, size_t b_stride);
// ---- what the loops of the LOD space (slod_lod_time.hip, slod_lod_wave.hip) are written on, once per scheme
// The operator of a column of a coarse multi-vector: one matrix for all columns, or (per_col) for column k member k of an
// ensemble matrix with leading dimension ld_m (include/slod.h).
struct SlodLodOperator
{
  const double *values;
  size_t        ld_m = 1;
  bool          per_col = false;
};
// Y = A X with the operator of every column: k_lod_apply (slod_lod_time.hip) or k_ens_apply (slod_lod_ensemble.hip)
inline void slod_lod_apply_launch(const slod_handle *h, hipStream_t st, const SlodLodOperator &A, const uint32_t *d_cols,
                                  const double *d_x, size_t ld_x, int n, double *d_y, size_t ld_y)
{
  if (A.per_col)
    slod_lod_apply_ensemble_launch(h, st, A.values, A.ld_m, d_cols, d_x, ld_x, n, d_y, ld_y);
  else
    slod_lod_apply_launch(h, st, A.values, d_cols, d_x, ld_x, n, d_y, ld_y);
}
// slod_check_ld for the n columns of a loop: below "n_rhs", or with a member per column below "n_members", the
// matrices' ld_m first
inline int slod_check_ld_of(const slod_handle *h, const char *who, bool per_col, std::initializer_list<size_t> ld_m, int n,
                            std::initializer_list<size_t> lds)
{
  const char *what = per_col ? "n_members" : "n_rhs";
  if (const int rc = per_col ? slod_check_ld(h, who, what, n, ld_m) : SLOD_OK)
    return rc;
  return slod_check_ld(h, who, what, n, lds);
}
// How a loop solves  S u = rhs  on its n columns: the recurrence of slod_lod_solve_multi, or the two sweeps of a factor the
// caller built, with all columns on its one member or with column k on member k.  The checks of a scheme take the kind
// for the wording of its call: an ensemble call names the handle among its NULL arguments and counts members.
enum SlodLodSolveKind { SLOD_SOLVE_CG, SLOD_SOLVE_FACTOR, SLOD_SOLVE_FACTOR_PER_COL };
// The solve of a step and the one device allocation of the loop around it.  A loop on a factor is queued whole: solve()
// only launches, and nothing of the CG workspace or of its active flags is allocated.
struct SlodLodStepSolve
{
  SlodLodSolveKind kind;
  slod_lod_factor *f = nullptr; // on a factor: the caller's
  // CG: the matrix (a loop that builds S in its workspace sets it after alloc), the stopping rule, and the HOST arrays
  // [n_steps], either may be NULL, where solve(k, ..) records step k
  const uint32_t    *d_cols = nullptr;
  const double      *S = nullptr;
  double             rel_tol = 0.0;
  int                max_iterations = 0;
  int               *iterations = nullptr;
  double            *rel_residual = nullptr;
  SlodLodWork        work; // CG: the workspace; its last, worst and report() are those of the solves (0 on a factor)
  SlodDevBuf<double> buf;  // on a factor: the pieces of the loop

  bool cg() const { return kind == SLOD_SOLVE_CG; }
  // carve(SlodCarver &) names the pieces of the loop and calls take() where those of the solve go, as SlodLodWork::alloc:
  // CG that allocation (two hipMalloc), else one SlodDevBuf
  template <typename Carve>
  hipError_t alloc(int n, Carve &&carve)
  {
    if (cg())
      return work.alloc(n, carve);
    SlodCarver count, hand;
    carve(count);
    const hipError_t e = buf.alloc(count.used);
    if (e != hipSuccess)
      return e;
    hand.base = buf.get();
    carve(hand);
    return hipSuccess;
  }
  void take(SlodCarver &c, const slod_handle *h)
  {
    if (cg())
      work.take_solve(c, h);
  }
  // u = S^-1 rhs for the n columns, the solve of step k.  CG: every column from zero; synchronises h->stream (= st), then
  // records the iterations and the residual of step k.  Factor: launches on st; a failed launch shows at the caller's
  // next hipGetLastError.
  hipError_t solve(slod_handle *h, hipStream_t st, int k, int n, const double *d_rhs, size_t ld_rhs, double *d_u, size_t ld_u)
  {
    if (cg())
      {
        const hipError_t e = work.solve(h, S, d_cols, d_rhs, ld_rhs, d_u, ld_u, rel_tol, max_iterations);
        if (e == hipSuccess)
          work.record(k, iterations, rel_residual);
        return e;
      }
    if (kind == SLOD_SOLVE_FACTOR_PER_COL)
      slod_lod_factor_solve_launch(f, st, d_rhs, ld_rhs, 1, d_u, ld_u, 0, n);
    else
      slod_lod_factor_solve_launch(f, st, d_rhs, ld_rhs, n, d_u, ld_u);
    return hipSuccess;
  }
};
#endif
