/*
 * include/slod.h -- flat C-ABI of libslod_hip.so: the MI355X-native replacement for the
 * per-patch SLOD basis construction of camillabelponer/dealii-slod.
 *
 * The reference has no FFI; its boundary for this path is the C++ member function
 *     void LOD<dim,spacedim>::compute_basis_function_candidates()
 *         (reference include/LOD.h:175-176, source/LOD.cc:296-768)
 * reading  patches[id].cells / sub_tria, par.{n_global_refinements, n_subdivisions,
 *          oversampling, LOD_stabilization, constant_coefficients} and the problem's
 *          coefficient Function (include/Diffusion.h:68, include/Elasticity.h:111-113),
 * writing  patches[id].basis_function / basis_function_premultiplied
 *          (include/LOD.h:79-80, source/LOD.cc:592,754,764).
 * Every entry point below names the reference code it replaces.  INTEGRATION.md shows the
 * deal.II-side binding (the body a maintainer puts into source/LOD.cc).
 *
 * Conventions: plain C types only; return 0 on success, a negative slod_status otherwise
 * (never throws across the ABI; slod_last_error() gives the text -- the reference throws
 * deal.II exceptions instead, LODtools.h:416-438).  Caller owns every buffer it passes;
 * the library owns its device workspace.  A handle is thread-compatible (one thread at a
 * time), like the reference's non-re-entrant patch loop (LOD.cc:302-322).  A plan owns ONE
 * workspace and ONE status word: executes of the same plan must not overlap (enqueue them on
 * one stream, or wait for the previous one); different plans of a handle may run concurrently
 * on different streams.
 *
 * Vector layout: per patch, PATCH-LEXICOGRAPHIC node order, component-minor:
 *     dof = spacedim*(ix + iy*(nx+1)) + comp,  ix in [0,nx], iy in [0,ny], nx = n_sub*mx.
 * slod_patch_dof_permutation() maps it to the deal.II patch-local numbering that
 * Patch::basis_function uses (consumer: assemble_global_matrix, LOD.cc:931-962).
 */
#ifndef SLOD_H
#define SLOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLOD_ABI_VERSION 5

typedef enum
{
  SLOD_OK              = 0,
  SLOD_ERR_ARGUMENT    = -1, /* bad config / null pointer / id out of range        */
  SLOD_ERR_UNSUPPORTED = -2, /* dim != 2, spacedim not in {1,2}, patch too large    */
  SLOD_ERR_DEVICE      = -3, /* HIP runtime error (no GPU, launch failure, OOM)     */
  SLOD_ERR_STATE       = -4, /* coefficient not set, plan/handle mismatch           */
  SLOD_ERR_NUMERIC     = -5  /* non-positive pivot in a patch solve                 */
} slod_status;

/* The five scalars of LODParameters the path reads (include/LOD.h:85-157) + device. */
typedef struct
{
  int32_t dim;                   /* must be 2 (reference: source/LOD.cc:1470-1471)            */
  int32_t spacedim;              /* 1 = DiffusionProblem, 2 = ElasticityProblem               */
  int32_t n_global_refinements;  /* N = 2^n coarse cells per side, patches in Morton order    */
  int32_t n_cells_per_side;      /* 0, or N for a non-2^k grid (then row-major patch order)   */
  int32_t n_subdivisions;        /* FE_Q_iso_Q1(n) (LOD.cc:87-89)                             */
  int32_t oversampling;          /* LOD.cc:156-178                                            */
  int32_t lod_stabilization;     /* 1 = SLOD branch (LOD.cc:563-564)                          */
  int32_t constant_coefficients; /* quirk Q1: re-use first full patch matrix (LOD.cc:354-362) */
  int32_t projection_quirk;      /* quirk Q2: projection_P1_P0<2,2> row parity (LODtools.h:43-67) */
  int32_t n_problems;            /* >= 1 independent coefficient realisations (ensemble)      */
  int32_t device;                /* HIP device ordinal                                        */
  int32_t reserved;
} slod_config;

/* What create_patches()/create_mesh_for_patch() (LOD.cc:122-244,770-858) and
 * fill_dofs_indices_vector() (LODtools.h:334-375) produce for one patch. */
typedef struct
{
  int32_t cx, cy;          /* centre cell                                                   */
  int32_t x0, y0, mx, my;  /* patch extent in coarse cells                                  */
  int32_t nx, ny;          /* fine elements per side                                        */
  int32_t side_domain[4];  /* left,right,bottom,top: 1 = boundary id 0, 0 = id 99           */
  int32_t n_fine;          /* N_f  = spacedim*(nx+1)*(ny+1)                                 */
  int32_t n_internal;      /* N_I                                                           */
  int32_t n_boundary;      /* N_b  (id-99 dofs)                                             */
  int32_t n_coarse;        /* N_c  = spacedim*mx*my                                         */
  int32_t is_lod;          /* branch of LOD.cc:563-564 taken for this patch                 */
} slod_patch_info;

typedef struct slod_handle slod_handle;
typedef struct slod_plan   slod_plan;

int         slod_abi_version(void);
/* text of the last error on this handle (handle may be NULL: last slod_create failure). */
const char *slod_last_error(const slod_handle *h);

/* replaces LOD::LOD + make_grid + make_fe + initialize_patches (LOD.cc:12-31,65-119,1380-1393) */
int  slod_create(const slod_config *cfg, slod_handle **out);
void slod_destroy(slod_handle *h);

/* patches per problem = N*N (LOD.cc:237-242) */
int slod_num_patches(const slod_handle *h);
/* replaces create_patches + create_mesh_for_patch + fill_dofs_indices_vector for one patch */
int slod_patch_layout(const slod_handle *h, uint32_t patch_id, slod_patch_info *info);
/* patch->cells in the reference's order, centre first (LOD.cc:151-178); entries cx + N*cy */
int slod_patch_cells(const slod_handle *h, uint32_t patch_id, uint32_t *cells, size_t capacity);
/* perm[dealii_dof] = lexicographic dof, for DoFHandler::distribute_dofs(FESystem(FE_Q_iso_Q1(n),
 * spacedim)) on the patch sub_tria (LOD.cc:365-366); see DESIGN.md for the numbering rule. */
int slod_patch_dof_permutation(const slod_handle *h, uint32_t patch_id, uint32_t *perm,
                               size_t capacity);
/* Utilities::MPI::create_evenly_distributed_partitioning (LOD.cc:116-118) */
int slod_partition(uint64_t n_total, uint32_t n_ranks, uint32_t rank, uint64_t *begin,
                   uint64_t *end);

/* Coefficient field of problem `problem` (replaces Alpha/Lambda/Mu.value_list at the
 * quadrature points, Diffusion.h:154, Elasticity.h:208-209).  field 0 = alpha or lambda,
 * 1 = mu.  layout 0: one value per fine element, [NE][NE] row-major (ex fastest);
 * layout 1: four values per element, [NE][NE][4], q = q0 + 2*q1 of QIterated(QGauss<1>(2),n)
 * (LOD.cc:91-92).  NE = N*n_subdivisions.  `on_device` != 0: data is a device pointer. */
int slod_set_coefficient(slod_handle *h, uint32_t problem, int field, const double *data,
                         int layout, size_t count, int on_device);

/* ---- the hot path ------------------------------------------------------------------ */
/* A plan fixes the list of (global) patch ids  gid = problem*num_patches + patch_id  and
 * where each patch's result goes (offsets in doubles into basis/premult; NULL = uniform
 * stride slod_plan_stride()).  Replaces the loop header LOD.cc:345-352. */
int    slod_plan_create(slod_handle *h, const uint32_t *gids, size_t n, const uint64_t *offsets,
                        slod_plan **out);
void   slod_plan_destroy(slod_plan *p);
size_t slod_plan_stride(const slod_plan *p);       /* doubles per patch with NULL offsets   */
size_t slod_plan_output_size(const slod_plan *p);  /* doubles needed in basis (and premult) */
/* Runs the loop body LOD.cc:353-767 for every patch of the plan on the GPU.  d_basis /
 * d_premult are DEVICE pointers; per patch: spacedim vectors of n_fine doubles each
 * (= Patch::basis_function[d], Patch::basis_function_premultiplied[d]).  Asynchronous on
 * `hip_stream` (a hipStream_t, NULL = the handle's own stream). */
int slod_plan_execute(slod_plan *p, double *d_basis, double *d_premult, void *hip_stream);
/* Keep HIP-event records of the next `depth` executes (default 1 = the last one only);
 * resets the record.  The events sit on the stream the kernels are launched on. */
int slod_plan_profile(slod_plan *p, int depth);
/* mean per-kernel device time over the recorded executes (HIP events around every launch of
 * slod_plan_execute; slod_plan_execute_allgather records none: SLOD_ERR_STATE after it);
 * synchronises.  ms[0] assemble, ms[1] patch solve, ms[2] selection */
int slod_plan_kernel_ms(slod_plan *p, float ms[3]);
/* Overlap of consecutive executes inside the library (depth 1 = default, 2).  All workgroups of a step
 * start together and run through the same phases in lock-step; two steps half a phase apart fill each
 * other's idle issue slots (+14..16 % patches/s at BASELINE config C2).  With depth 2 the plan owns a
 * second workspace and two internal streams; slod_plan_execute alternates between them.  Each execute
 * is ordered AFTER everything submitted to its hip_stream so far, but hip_stream is NOT ordered after
 * the execute: call slod_plan_join(plan, stream) to make a stream wait for the executes in flight
 * (asynchronous), or slod_plan_status (synchronises).  Plans that run in several workspace chunks are
 * refused (SLOD_ERR_STATE): their launches de-phase by themselves.  Reference: the serial patch loop
 * LOD.cc:345-767 has no counterpart. */
int slod_plan_set_overlap(slod_plan *p, int depth);
int slod_plan_join(slod_plan *p, void *hip_stream);
/* The k-th patch descriptor the plan's kernels LAUNCH with, read back from the device (the descriptors
 * are produced by a device kernel from the grid scalars: create_patches + create_mesh_for_patch,
 * LOD.cc:122-244,770-858).  launch_order = 0: the caller's order; 1: the balanced launch order
 * (plan_index then tells which entry of the caller's list sits at launch position k). */
int slod_plan_patch_layout(slod_plan *p, size_t k, int launch_order, slod_patch_info *info, uint32_t *plan_index);
/* numerical status of the last execute (0 or SLOD_ERR_NUMERIC); synchronises.
 * SLOD_ERR_NUMERIC (here and from slod_compute_basis): at least one patch of the last execute met a pivot that is
 * not positive or not finite, in its patch solve or in the inversion of M = P^T A^-1 P (an indefinite or singular
 * patch matrix, NaN or Inf in the coefficient).  ALL outputs and diagnostics of that execute are undefined, those
 * of the other patches included: the kernels read the workspace of neighbouring patches unchecked.  (The
 * reference aborts the whole run here: AssertThrow after the patch solve, LODtools.h:416-428.)
 * The plan and the handle remain usable: the next execute on valid coefficients gives the results of a fresh
 * plan, bit for bit (it starts by zero-filling the workspace the failed one left; no host synchronisation).
 * With slod_plan_set_overlap(2) the status covers the most recent execute of EACH of the two workspaces:
 * directly after a failed execute and ONE good one it still reports the failure, after two good ones it is 0. */
int slod_plan_status(slod_plan *p);

/* Decisions the SLOD selection stage took for one (patch, component): the discontinuous part
 * of LOD.cc:656-725 (pseudo-inverse cutoff :667, "drop the smallest triplet while
 * ||d||_inf >= 0.5" :703-725).  Parity tests assert them equal to the CPU oracle's. */
typedef struct
{
  int32_t path;       /* 0 = LOD branch (LOD.cc:566-595); 1 = SLOD, proven decision-free (QR:
                         no singular value near the cutoff, ||d||_inf < 0.5); 2 = SLOD, loop
                         replayed on the singular triplets                                     */
  int32_t n_cut;      /* singular values of G = BD'^T BD' with sigma <= 1e-15 sigma_0 (:667)   */
  int32_t n_dropped;  /* triplets put back by the 0.5-loop (:703-725)                          */
  int32_t sweeps;     /* Jacobi sweeps of the replay (path 2)                                  */
  double  dinf;       /* final ||d||_inf                                                       */
  double  sigma_max, sigma_min; /* extreme singular values of G (path 2; 0 otherwise)          */
} slod_patch_diag;
/* out[k*spacedim + d] for patch k of the plan, component d, of the LAST execute; HOST buffer of
 * `capacity` entries.  Returns the number of entries written or a negative slod_status;
 * synchronises. */
int slod_plan_diagnostics(slod_plan *p, slod_patch_diag *out, size_t capacity);

/* Host-buffer convenience wrapper: plan + execute + copy back (what the deal.II adapter
 * calls).  basis/premult are HOST pointers. */
int slod_compute_basis(slod_handle *h, const uint32_t *gids, size_t n, double *basis,
                       double *premult, const uint64_t *offsets);

/* ---- consumers of (phi, psi): the global LOD system ----------------------------------
 * Reference: assemble_global_matrix (LOD.cc:860-973), solve (LOD.cc:976-1002), and the
 * fine-scale reconstruction  solution_fine = C u_H  (LOD.cc:1251).  All vectors of ONE problem
 * sit in a slab with uniform stride (slod_plan_stride(): what a plan with NULL offsets
 * writes and what the all-gather of the multi-GPU path produces): patch p at
 * d_basis[p * stride + d * n_fine(p) + dof].  Overlaps of patches are index arithmetic on
 * the patch-lexicographic layout; no deal.II numbering is involved.  Any stride >= s * max_p n_fine(p)
 * is accepted: the words of a patch between its s vectors and the stride are never read. */
/* Upper bound of patches q whose node set meets that of one patch: (4 l + 3)^2 (the closed patches
 * of two cells share a node as soon as their centres are at most 2 l + 1 cells apart per axis). */
int slod_lod_row_capacity(const slod_handle *h);
/* Patches coupled with `patch_id` in A_LOD (LOD.cc:970-971 pattern of Tmmult), ascending ids;
 * returns their count.  HOST buffer. */
int slod_lod_pattern(const slod_handle *h, uint32_t patch_id, uint32_t *neighbours, size_t capacity);
/* Block rows of  A_LOD = C^T (A C)  (basis_matrix_transposed.Tmmult(global_stiffness_matrix,
 * premultiplied_basis_matrix), LOD.cc:970-971) for the patches rows[0..n_rows):
 *   d_values[(k * cap + j) * s * s + d * s + e] = sum_i phi_{rows[k],d}(i) psi_{q,e}(i),
 *   q = d_cols[k * cap + j]  (0xffffffff = unused slot), cap = slod_lod_row_capacity().
 * Column (q,e) of the reference matrix is spacedim * q + e (LOD.cc:942-944).  rows is a HOST
 * array; d_* are DEVICE pointers.  The call uploads the row list (a device allocation of its own) and
 * returns after hip_stream has finished the kernel: it SYNCHRONISES hip_stream. */
int slod_lod_matrix(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis,
                    const double *d_premult, size_t stride, double *d_values, uint32_t *d_cols,
                    void *hip_stream);
/* system_rhs = C^T fem_rhs (basis_matrix_transposed.Tvmult, LOD.cc:982): d_out[k * s + d] =
 * sum_i phi_{rows[k],d}(i) f(i); d_fine_rhs is the fine FEM load vector on the GLOBAL fine
 * grid, [(NE+1)^2][s] lexicographic, component-minor. */
int slod_lod_rhs(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, size_t stride,
                 const double *d_fine_rhs, double *d_out, void *hip_stream);
/* Solves A_LOD u = rhs for all num_patches * s unknowns (the reference: CG + SSOR(1.2),
 * LOD.cc:990-998; here Jacobi-preconditioned CG, all on the device) from the block rows of
 * slod_lod_matrix for rows = 0 .. num_patches-1.  Returns the iteration count (>= 0) or a
 * negative slod_status; *rel_residual (HOST, may be NULL) receives ||r|| / ||rhs||.  Synchronises. */
int slod_lod_solve(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_rhs,
                   double *d_u, double rel_tol, int max_iterations, double *rel_residual);
/* solution_fine = C u_H (LOD.cc:1251: basis_matrix_transposed.vmult): d_fine[(ix + iy (NE+1)) s + c]
 * = sum over patches covering the node, sum_d phi_{p,d}(node, c) u[p s + d]. */
int slod_lod_reconstruct(slod_handle *h, const double *d_basis, size_t stride, const double *d_u,
                         double *d_fine, void *hip_stream);

/* ---- the same three steps for n_rhs load vectors at once -----------------------------
 * The basis is built once and serves many right-hand sides (load cases, time steps, parameter studies):
 * one call per step for all of them instead of n_rhs calls (the reference solves a single load,
 * LOD.cc:976-1002).  slod_lod_rhs, slod_lod_solve and slod_lod_reconstruct are the case n_rhs = 1.
 * Layouts:
 *   fine multi-vector    n_rhs fields, each in the layout of the single-vector call ([(NE+1)^2][s],
 *                        lexicographic, component-minor); field c starts at base + c * ld_fine,
 *                        ld_fine >= (NE+1)^2 * s.  A field is what slod_fem_rhs writes.
 *   coarse multi-vector  (d_out, d_rhs, d_u) interleaved: entry (i, c) of the num_patches * s unknowns at
 *                        base[i * ld + c], ld >= n_rhs: the n_rhs values of one row are contiguous, which is
 *                        what lets the matrix product read them coalesced.  n_rhs = 1, ld = 1 is the
 *                        single-vector layout; a column sub-range of a wider array is base + first column.
 * Entries c >= n_rhs inside a row's ld are never read or written.  SLOD_ERR_ARGUMENT (before any device work):
 * NULL handle or array, n_rhs < 1, ld < n_rhs, ld_fine shorter than a field, max_iterations < 0. */
/* d_out[(k * s + d) * ld_out + c] = sum_i phi_{rows[k],d}(i) f_c(i)  (slod_lod_rhs per column, bit for bit).
 * SYNCHRONISES hip_stream (the row list is uploaded, as in slod_lod_rhs). */
int slod_lod_rhs_multi(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, size_t stride,
                       const double *d_fine_rhs, size_t ld_fine, int n_rhs,
                       double *d_out, size_t ld_out, void *hip_stream);
/* A_LOD u_c = rhs_c for every column c.  Each column runs the Jacobi-preconditioned CG recurrence of
 * slod_lod_solve with its own alpha, beta, r.z and r.r, from u = 0, and has converged when
 * r.r <= rel_tol^2 ||rhs_c||^2; that is checked every 8 iterations (the last burst is min(8, max_iterations - it)).
 * These are n_rhs independent recurrences that share the reads of the matrix and the kernel launches (three per
 * iteration for all columns), not a block-Krylov method.  A column that passes its check is frozen: its u is not
 * written again.  A zero column gives u = 0, 0 iterations, residual 0.  The loop ends when every column is frozen
 * or at max_iterations (not an error, as in slod_lod_solve).
 * Dot products are summed in a fixed order (no atomics): the bits of column c of d_u, and iterations[c], depend
 * only on the matrix and on column c of d_rhs -- not on n_rhs, the column's position, ld, the other columns or
 * the run.  Any n_rhs >= 1; device workspace of 4 * num_patches * s * n_rhs doubles, allocated per call.
 * Returns the largest per-column iteration count or a negative slod_status; iterations[c] and rel_residual[c]
 * = ||r_c|| / ||rhs_c|| are HOST arrays of n_rhs entries (either may be NULL).  Runs on the handle's stream;
 * synchronises. */
int slod_lod_solve_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols,
                         const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u, size_t ld_u,
                         double rel_tol, int max_iterations,
                         int *iterations /* HOST [n_rhs], may be NULL */,
                         double *rel_residual /* HOST [n_rhs], may be NULL */);
/* field c of d_fine = C u_c (slod_lod_reconstruct on column c, bit for bit: the covering patches are
 * visited in the same order).  Asynchronous on hip_stream. */
int slod_lod_reconstruct_multi(slod_handle *h, const double *d_basis, size_t stride,
                               const double *d_u, size_t ld_u, int n_rhs,
                               double *d_fine, size_t ld_fine, void *hip_stream);

/* ---- the L2 inner product on the LOD space and a time loop on it ----------------------
 * The reference solves one stationary problem (LOD.cc:976-1002) and has no counterpart of this block.  With
 * M_LOD = C^T M_rho C the basis serves parabolic problems (M u' + A u = b), the eigenvalue problem
 * A_LOD u = lambda M_LOD u, and, through slod_lod_apply_multi and slod_lod_matrix_combine, any scheme a host builds
 * from products and linear combinations of the two matrices.  Every matrix below is a full set of block rows in the
 * layout of slod_lod_matrix; coarse multi-vectors are those of the _multi calls (entry (i, c) at base[i * ld + c]).
 * Common: argument checks come before any device work (SLOD_ERR_ARGUMENT); SLOD_ERR_DEVICE without a usable GPU. */
/* Block rows of M_LOD for the patches rows[0..n_rows), layout and pattern of slod_lod_matrix:
 *   d_values[(k * cap + j) * s * s + d * s + e] = sum_c int rho phi_{rows[k],d,c} phi_{q,e,c} dx,  q = d_cols[k * cap + j],
 * cap = slod_lod_row_capacity(), unused slots 0xffffffff with value 0.  For the same rows d_cols equals what
 * slod_lod_matrix writes, word for word: a pair of patches that shares only a line of nodes keeps its column, here
 * with the value 0.  Components do not couple in the mass; block (d, e) is the sum over c above.
 * The integral is the consistent Q1 mass of the global fine grid, element matrix
 *   rho_e h^2 / 36 [[4,2,2,1],[2,4,1,2],[2,1,4,2],[1,2,2,4]],  h = 1 / NE  (nodes (0,0), (1,0), (0,1), (1,1)),
 * summed over the fine elements of the intersection rectangle of the two closed patches, which is the global form
 * because phi vanishes on every patch rim.  d_rho: DEVICE [NE][NE], one value per fine element, ex fastest (layout 0 of
 * slod_set_coefficient), an argument and not handle state; NULL = 1.  Only the basis slab is read (d_basis, stride as
 * in slod_lod_matrix).  The sum has a fixed order (no atomics): the same inputs give the same bits, and
 * M[(p,d),(q,e)] and M[(q,e),(p,d)] are the same bits when both rows are computed.  rows is a HOST array, ids
 * < num_patches; the call uploads it and SYNCHRONISES hip_stream, like slod_lod_matrix. */
int slod_lod_mass_matrix(slod_handle *h, const uint32_t *rows, size_t n_rows, const double *d_basis, size_t stride,
                         const double *d_rho, double *d_values, uint32_t *d_cols, void *hip_stream);
/* Y = A X for a full set of block rows (rows = 0 .. num_patches-1 of slod_lod_matrix or slod_lod_mass_matrix, or a
 * combination of them): d_y[i * ld_y + c] = sum_j sum_e values[...] d_x[(q s + e) * ld_x + c].  n_rhs = 1, ld = 1 is
 * the single-vector product.  One fma chain per entry over the slots of the row in ascending order: the bits of
 * column c of Y depend only on the matrix and on column c of X, not on n_rhs, ld or the column's position.  Entries
 * c >= n_rhs of a row are never read or written.  SLOD_ERR_ARGUMENT: NULL handle or array, n_rhs < 1, ld < n_rhs,
 * d_x == d_y (the product cannot run in place).  Asynchronous on hip_stream. */
int slod_lod_apply_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                         int n_rhs, double *d_y, size_t ld_y, void *hip_stream);
/* d_out = alpha A + beta B on the values arrays of two full sets of block rows that share one d_cols (which the call
 * does not need): per entry  out = (alpha * a) + (beta * b)  with the two products and the sum rounded separately (no
 * fma), which is what `alpha * A + beta * B` gives in numpy.  Unused slots stay 0.  d_out may be d_a or d_b.
 * Asynchronous on hip_stream. */
int slod_lod_matrix_combine(slod_handle *h, double alpha, const double *d_a, double beta, const double *d_b, double *d_out,
                            void *hip_stream);
/* n_steps steps of the theta scheme for  M u' + A u = b(t)  on n_rhs independent columns (initial states and / or loads),
 * the whole loop on the device.  In increment form, for k = 0 .. n_steps-1:
 *   S = M + theta dt A                                   (slod_lod_matrix_combine, once per call, workspace of the call)
 *   g = (theta b^{k+1} + (1 - theta) b^k) - A u^k        (slod_lod_apply_multi; products and sums rounded separately)
 *   S delta = dt g                                        (the recurrence of slod_lod_solve_multi from delta = 0, per-column
 *                                                          freeze, rel_tol relative to ||dt g_c||, checked every 8 iterations)
 *   u^{k+1} = u^k + delta
 * theta = 1: backward Euler; 1/2: Crank-Nicolson; 0: forward Euler (S = M).  d_stiffness, d_mass: values arrays of
 * slod_lod_matrix and slod_lod_mass_matrix for rows = 0 .. num_patches-1, d_cols their common columns.  d_u: u^0 on
 * entry, u^{n_steps} on return (ld_u >= n_rhs).  d_load: the coarse loads b^k = C^T f(t_k), k = 0 .. n_steps, b^k at
 * d_load + k * load_step_stride (doubles) with ld_load >= n_rhs; load_step_stride = 0: one load, constant in time;
 * d_load = NULL: zero load (ld_load, load_step_stride ignored).  A zero column of dt g gives delta = 0 and 0 iterations;
 * reaching max_iterations is not an error.  HOST iterations[n_steps]: the largest per-column iteration count of each
 * step; HOST rel_residual[n_steps]: the worst column's ||r|| / ||dt g|| of each step; either may be NULL.  Returns the
 * largest entry of iterations or a negative slod_status.  The bits of column c of the result depend only on the two
 * matrices, the parameters, and column c of u^0 and of the loads; one call with n_steps = 2 equals two calls with
 * n_steps = 1.  Device workspace (one matrix, 6 vectors of n_rhs columns) allocated once per call.
 * SLOD_ERR_ARGUMENT: NULL handle, matrix, d_cols or d_u; dt <= 0; theta outside [0, 1]; n_steps < 1; n_rhs < 1;
 * ld_u < n_rhs; ld_load < n_rhs with a load; max_iterations < 0.  Runs on the handle's stream; synchronises.  A record
 * armed by slod_lod_time_record_arm (below) is taken by this call: the trace of u at the receivers, on the device. */
int slod_lod_theta_steps(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double dt,
                         double theta, int n_steps, int n_rhs, double *d_u, size_t ld_u, const double *d_load, size_t ld_load,
                         size_t load_step_stride, double rel_tol, int max_iterations,
                         int *iterations /* HOST [n_steps], may be NULL */,
                         double *rel_residual /* HOST [n_steps], may be NULL */);

/* ---- the eigenvalue problem  A_LOD u = lambda M_LOD u  on the device ---------------------
 * The lowest vibration modes or heat-decay rates of the medium, on the LOD space (the reference has no counterpart).
 * Matrices are full sets of block rows (rows 0 .. num_patches-1) in the layout of slod_lod_matrix, coarse multi-vectors
 * those of the _multi calls.  Argument checks come before any device work; SLOD_ERR_DEVICE without a usable GPU. */
/* d_out = (A + A^T) / 2 on the block rows: for every used slot (p, j), q = d_cols[p * cap + j], and every (d, e)
 *   d_out[(p * cap + j) * s * s + d * s + e] = 0.5 * (A[p,j][d][e] + A[q,j'][e][d]),  j' the slot of p in row q
 * (0 for the transposed entry if row q does not hold p; the pattern of slod_lod_matrix is symmetric).  The sum is
 * rounded once and the halving is exact, so d_out is symmetric bit for bit and equals numpy's 0.5 * (A + A.T) of the
 * densified rows bit for bit.  Unused slots are written as +0.  slod_lod_matrix gives A_LOD symmetric only up to the
 * basis accuracy (~1e-9 of its scale); that skew part would set a floor under every eigen-residual.
 * SLOD_ERR_ARGUMENT: NULL handle or array; d_out == d_values (a row reads other rows, the call cannot run in place).
 * Asynchronous on hip_stream. */
int slod_lod_matrix_symmetrize(slod_handle *h, const double *d_values, const uint32_t *d_cols, double *d_out, void *hip_stream);
/* The lowest n_eig eigenpairs of the symmetric pencil (A, M) by block inverse iteration with Rayleigh-Ritz on
 * m = n_block columns, 1 <= n_eig <= n_block <= min(64, num_patches * s); the n_block - n_eig extra columns are guard
 * vectors (the error of column j contracts by about lambda_j / lambda_{m+1} per outer iteration).
 * d_stiffness must be symmetric: the output of slod_lod_matrix_symmetrize (not checked).  d_mass: the output of
 * slod_lod_mass_matrix, which is bit-symmetric already.
 * start = 1: d_x holds the start block on entry.  start = 0: the call writes one: column j, with t = j / s and
 * d = j % s, has the entry  delta_de sin(a_t pi (cx + 1/2) / N) sin(b_t pi (cy + 1/2) / N)  for (patch p, component e),
 * (cx, cy) the centre cell of p and (a_t, b_t) the t-th pair of {1..N}^2 in ascending a^2 + b^2, ties by ascending a
 * (the discrete sine modes on the cell centres).
 * Outer iteration k = 1, 2, ..; only the n_block residuals and the inner solve's flags are read back per iteration:
 *   Y = M X;  A Z = Y from Z = 0 (the recurrence of slod_lod_solve_multi with inner_rel_tol, inner_max_iterations);
 *   W = A Z, V = M Z (exact products: the residual below is honest whatever the inner tolerance was);
 *   Ga = sym(Z^T W), Gm = sym(Z^T V);  Ga Q = Gm Q Theta with Q^T Gm Q = I, Theta ascending (Cholesky of Gm,
 *   cyclic Jacobi);  X = Z Q;  res_j = ||A X_j - theta_j M X_j||_2 / (theta_j ||M X_j||_2) from W Q and V Q;
 *   stop when res_j <= tol for all j < n_eig, or at k = max_outer (not an error, as in slod_lod_solve).
 * On return d_x holds X, M-orthonormal, column j at d_x[i * ld_x + j] (entries j >= n_block of a row are never read or
 * written); HOST eigenvalues[n_block] and residuals[n_block] hold all n_block columns: the guard columns
 * j >= n_eig are less converged than the first n_eig and their residuals are not bounded by tol.
 * HOST inner_iterations[k] (max_outer entries, may be NULL): the largest per-column CG count of outer iteration k + 1.
 * Returns the number of outer iterations run (>= 1) or a negative slod_status.  SLOD_ERR_NUMERIC: a pivot of the
 * Cholesky of Gm is not above 4 m eps times its diagonal entry (rank-deficient block, e.g. two equal start columns);
 * d_x then holds the block the failed iteration started from.
 * Sums have a fixed order (no atomics): the same inputs give the same bits of X, Theta, the residuals and all counts,
 * run after run.  Unlike the _multi calls this is a block method: the columns are NOT independent of each other, a
 * column's result depends on n_block and on the other columns.  Device workspace (8 vectors of n_block columns and the
 * slab partials of the Gram products) allocated once per call.
 * SLOD_ERR_ARGUMENT: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals; n_eig < 1; n_block < n_eig;
 * n_block > 64 or > num_patches * s; ld_x < n_block; start not 0 or 1; tol or inner_rel_tol <= 0 or NaN; max_outer < 1;
 * inner_max_iterations < 0.  Runs on the handle's stream; synchronises. */
int slod_lod_eigs(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                  int n_eig, int n_block, int start, double *d_x, size_t ld_x,
                  double tol, int max_outer, double inner_rel_tol, int inner_max_iterations,
                  double *eigenvalues      /* HOST [n_block] */,
                  double *residuals        /* HOST [n_block] */,
                  int    *inner_iterations /* HOST [max_outer], may be NULL */);

/* ---- second-order time stepping on the LOD space:  M u'' + C u' + A u = b(t)  -------------
 * Wave propagation through the medium, with Rayleigh damping C = damp_mass M + damp_stiff A (the reference has no
 * counterpart).  Matrices are full sets of block rows (rows 0 .. num_patches-1) in the layout of slod_lod_matrix, coarse
 * multi-vectors those of the _multi calls.  d_stiffness should be the output of slod_lod_matrix_symmetrize (not
 * checked, as in slod_lod_eigs): the energy identities of the scheme hold for a symmetric A.  Argument checks come
 * before any device work; SLOD_ERR_DEVICE without a usable GPU. */
/* out[c] = sum_i x[i,c] (A y)[i,c], the bilinear form of a block-row matrix per column; d_x == d_y gives the quadratic
 * form (u^T A u, v^T M v).  (A y)[i,c] is the fma chain of slod_lod_apply_multi (the same bits); the product with
 * x[i,c] is rounded on its own; the sum has the fixed order of slod_lod_solve_multi: the 16 rows of a group ascending
 * into one partial per (group, column), then the partials in ascending group order (a second, per-column launch).  No
 * atomics: the bits of out[c] depend only on the matrix and on column c of x and y, not on n_rhs, ld, the column's
 * position or the run.  SLOD_ERR_ARGUMENT: NULL handle or array, n_rhs < 1, ld < n_rhs.  Synchronises hip_stream. */
int slod_lod_inner_multi(slod_handle *h, const double *d_values, const uint32_t *d_cols, const double *d_x, size_t ld_x,
                         const double *d_y, size_t ld_y, int n_rhs, double *out /* HOST [n_rhs] */, void *hip_stream);
/* The acceleration consistent with a state (u, v) and the load b^0, per column:
 *   M a = b^0 - A (u + damp_stiff v) - damp_mass M v
 * by the recurrence of slod_lod_solve_multi from a = 0 (per-column freeze, rel_tol relative to the norm of the
 * right-hand side; a zero column gives a = 0 and 0 iterations).  d_load = NULL: b^0 = 0 (ld_load ignored).  u and v are
 * read only.  Returns the largest per-column iteration count or a negative slod_status; reaching max_iterations is not
 * an error.  SLOD_ERR_ARGUMENT: NULL handle, matrix, d_cols, u, v or a; a negative or NaN damping coefficient;
 * n_rhs < 1; a leading dimension below n_rhs (ld_load only with a load); max_iterations < 0.  Runs on the handle's
 * stream; synchronises. */
int slod_lod_newmark_accel(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                           double damp_mass, double damp_stiff, int n_rhs, const double *d_u, size_t ld_u,
                           const double *d_v, size_t ld_v, const double *d_load /* b^0, NULL = 0 */, size_t ld_load,
                           double *d_a, size_t ld_a, double rel_tol, int max_iterations,
                           int *iterations /* HOST [n_rhs], may be NULL */,
                           double *rel_residual /* HOST [n_rhs], may be NULL */);
/* n_steps of Newmark-beta in acceleration form on n_rhs independent columns, the whole loop on the device.  On entry
 * u, v, a hold the state at level k0 (a from slod_lod_newmark_accel, or from the previous call), on return the state
 * n_steps later.  For k = 0 .. n_steps-1:
 *   S  = (1 + gamma dt damp_mass) M + (beta dt^2 + gamma dt damp_stiff) A     (once per call, workspace of the call)
 *   u~ = u + dt v + dt^2 (1/2 - beta) a ;  v~ = v + dt (1 - gamma) a           (predictor, in place)
 *   g  = b^{k+1} - A (u~ + damp_stiff v~) - damp_mass M v~
 *   S a+ = g                                 (the recurrence of slod_lod_solve_multi from 0, rel_tol relative to ||g_c||)
 *   u+ = u~ + beta dt^2 a+ ;  v+ = v~ + gamma dt a+
 * gamma = 1/2, beta = 1/4: the trapezoidal rule (unconditionally stable, conserves v^T M v / 2 + u^T A u / 2 without
 * load and damping).  gamma = 1/2, beta = 0: central differences (S is a multiple of M when damp_stiff = 0; stable for
 * omega_max dt < 2).  For 0 < beta < 1/4 the limit is omega_max dt < 2 / sqrt(1 - 4 beta).  Every solve starts from
 * zero (no warm start from a): a column's bits depend only on the matrices, the parameters and that column's state and
 * loads, and one call with n_steps = 2 equals two calls with n_steps = 1 carrying u, v, a over.  Products and sums of
 * the elementwise work are rounded separately (no fma).
 * d_load: b^k at d_load + k * load_step_stride (doubles), k = 0 .. n_steps, ld_load >= n_rhs, as in
 * slod_lod_theta_steps; step k reads b^{k+1} only; load_step_stride = 0: one load, constant in time; NULL: zero load.
 * HOST iterations[n_steps] / rel_residual[n_steps]: the largest per-column iteration count and the worst column's
 * ||r|| / ||g|| of each step.  HOST kinetic / potential [(n_steps + 1) * n_rhs]: entry [k * n_rhs + c] is
 * v_c^T M v_c / 2 and u_c^T A u_c / 2 (the sums of slod_lod_inner_multi, halved), k = 0 the entry state, k = 1 .. n_steps
 * the state after each step; kept on the device and copied once at the end; both NULL: not computed.
 * Returns the largest entry of iterations or a negative slod_status; reaching max_iterations is not an error.  Device
 * workspace (one matrix, 6 vectors of n_rhs columns, the energies) allocated once per call.
 * SLOD_ERR_ARGUMENT: NULL handle, matrix, d_cols, u, v or a; dt <= 0 or NaN; beta outside [0, 1/2] or gamma outside
 * [0, 1]; a negative or NaN damping coefficient; n_steps < 1; n_rhs < 1; a leading dimension below n_rhs (ld_load only
 * with a load); max_iterations < 0; exactly one of kinetic / potential given.  Runs on the handle's stream; synchronises.
 * A record armed by slod_lod_time_record_arm (below) is taken by this call: the traces of u and / or v at the receivers. */
int slod_lod_newmark_steps(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols, double dt,
                           double beta, double gamma, double damp_mass, double damp_stiff, int n_steps, int n_rhs,
                           double *d_u, size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a,
                           const double *d_load, size_t ld_load, size_t load_step_stride, double rel_tol, int max_iterations,
                           int *iterations      /* HOST [n_steps], may be NULL */,
                           double *rel_residual /* HOST [n_steps], may be NULL */,
                           double *kinetic      /* HOST [(n_steps + 1) * n_rhs], may be NULL */,
                           double *potential    /* HOST [(n_steps + 1) * n_rhs], may be NULL */);

/* ---- a direct solver on the LOD space: banded Cholesky, factor once, solve many --------------
 * The systems of the LOD space are small and, inside a time loop, never change.  In row-major cell order a block row
 * (slot j = the neighbour at cell offset (j % span, j / span) - span / 2, span = 4 l + 3) is a band of half width
 *   b = s (w N + w) + s - 1,  w = 2 l + 1,
 * and  A = L L^T  in band storage serves every later solve with two sweeps and no tolerance to tune (the reference has
 * no counterpart).  Factor ordering: unknown (p, d) has the index r = (cy N + cx) s + d, (cx, cy) the centre cell of
 * patch p, for Morton and for row-major patch ids alike; the permutation is internal, callers keep their patch order. */
typedef struct slod_lod_factor slod_lod_factor;
typedef struct
{
  int32_t  n, half_bandwidth, block; /* rows; b above; the edge of the square tiles of the band (16)                  */
  uint64_t bytes;                    /* device bytes the factor owns                                                  */
  double   min_pivot, max_pivot;     /* the smallest and largest diagonal entry of L, squared; of an LDL^T factor (below)
                                        the smallest and largest entry of D, signed                                   */
} slod_lod_factor_info;
/* Factors a symmetric positive definite matrix given as a full set of block rows (rows 0 .. num_patches-1 in the layout
 * of slod_lod_matrix: the output of slod_lod_matrix_symmetrize, slod_lod_mass_matrix, or a slod_lod_matrix_combine of
 * the two).  ONLY THE LOWER TRIANGLE IN FACTOR ORDER IS READ: an entry ((p, d), (q, e)) with r(q, e) <= r(p, d), taken
 * from the block row of its row's patch p; for a bit-symmetric input that makes no difference.  Allocates everything the
 * factor will ever need (the band in 16 x 16 tiles, at most about 8 n (b + 48) bytes), runs on the handle's stream (one launch
 * per block column of 16, queued without a host wait) and synchronises.
 * SLOD_ERR_NUMERIC: a pivot is not > 0 (an indefinite matrix, NaN in the input); slod_last_error names the call and the
 * index r of the first such pivot; *out stays NULL and nothing stays allocated.  SLOD_ERR_ARGUMENT (before any device
 * work): NULL handle, array or out.  SLOD_ERR_DEVICE without a usable GPU.  The factor belongs to the handle and must be
 * destroyed before it. */
int slod_lod_factor_create(slod_handle *h, const double *d_values, const uint32_t *d_cols, slod_lod_factor **out);
int slod_lod_factor_get_info(const slod_lod_factor *f, slod_lod_factor_info *info);
/* U = A^-1 RHS for n_rhs >= 1 columns, coarse multi-vectors of the _multi calls (entry (i, c) at base[i * ld + c], rows
 * in the caller's patch order).  d_u == d_rhs is allowed.  Asynchronous on hip_stream (NULL: the handle's); allocates
 * nothing and reads nothing back, so it can be captured like slod_plan_execute.  Entries c >= n_rhs of a row are never
 * read or written.  One block per 16 columns walks the block rows forwards, then backwards; every sum has a fixed order
 * (no atomics): the bits of column c of U depend only on the factor and on column c of RHS, not on n_rhs, an ld, the
 * column's position or the run.  The intermediate vector of the sweeps lives in d_u.  The factor is read only: solves
 * on several streams may share it.  SLOD_ERR_ARGUMENT: NULL factor or array, n_rhs < 1, ld < n_rhs. */
int slod_lod_factor_solve(slod_lod_factor *f, const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u, size_t ld_u,
                          void *hip_stream);
/* Waits for the handle's stream, then frees the factor.  NULL is allowed. */
void slod_lod_factor_destroy(slod_lod_factor *f);
/* ---- banded LDL^T: symmetric indefinite matrices, inertia ---------------------------------------
 * S = L D L^T, L unit lower triangular, D diagonal, 1 x 1 pivots, NO PIVOTING, in the band storage, the ordering and the
 * launch shape of slod_lod_factor_create (a permutation would destroy the band; LAPACK has no banded symmetric indefinite
 * routine either).  Meant for  S = sym(A) - sigma M  with sigma inside the spectrum (slod_lod_matrix_combine(1, sym A,
 * -sigma, M)): Helmholtz-type systems, shift-and-invert, and the count of eigenvalues below sigma.  Without pivoting the
 * factorisation is backward stable only relative to  G = || |L| |D| |L^T| ||_inf  in place of ||S||_inf; the factor
 * measures G (slod_lod_factor_inertia) so that the caller can judge it: a solve has a backward error of about
 * (3 (b + 1) + 1) (b + 1) 2^-53 G / ||S||_inf relative to ||S||_inf.
 * Every call that takes a factor takes an LDL^T factor unchanged: slod_lod_factor_solve and _solve_ensemble (L y = b,
 * L^T x = D^-1 y, the same fixed order of summation: the bits of a column depend on the factor and that column only),
 * slod_lod_theta_steps_direct, slod_lod_newmark_accel_direct, slod_lod_newmark_steps_direct and their _ensemble forms,
 * slod_lod_eigs_direct and slod_lod_eigs_ensemble_direct (their duty sigma < lambda_1 stays; with an interior shift use
 * slod_lod_eigs_shift_direct below).
 * slod_lod_factor_get_info(_member) reports min_pivot / max_pivot as the smallest and largest entry of D, signed.
 * SLOD_ERR_NUMERIC: a pivot is zero, infinite or NaN; slod_last_error reads
 *   "<call>: [member k: ]pivot r of n is zero or not finite (value)";
 * *out stays NULL and nothing stays allocated.  The other returns, and bad_pivot of the ensemble form, are
 * those of slod_lod_factor_create / slod_lod_factor_create_ensemble; member k's factor has the bits of
 * slod_lod_factor_create_ldl on its de-interleaved matrix. */
int slod_lod_factor_create_ldl(slod_handle *h, const double *d_values, const uint32_t *d_cols, slod_lod_factor **out);
int slod_lod_factor_create_ldl_ensemble(slod_handle *h, const double *d_values, size_t ld_m, int n_members,
                                        const uint32_t *d_cols, int32_t *bad_pivot /* HOST [n_members], may be NULL */,
                                        slod_lod_factor **out);
typedef struct
{
  int32_t n_negative, n_positive;     /* signs of D over the n real rows; n_negative = eigenvalues of (A, M) below sigma
                                         when S = sym(A) - sigma M and M is positive definite (Sylvester)            */
  double  min_abs_pivot, max_abs_pivot;
  double  norm_matrix, norm_factor;   /* ||S||_inf and || |L||D||L^T| ||_inf; their ratio is the growth              */
} slod_lod_factor_inertia_info;
/* The inertia and the growth of member `member` of an LDL^T factor (a single factor has the member 0), from the read-back
 * of the create call: no device work.  norm_matrix is the row-sum norm of the symmetric matrix whose lower triangle was
 * read, norm_factor = max_i (|L| (|D| (|L^T| e)))_i, both over the n real rows in factor order with fixed-order sums.
 * norm_factor is an ORDER-OF-MAGNITUDE DIAGNOSTIC, promised to a factor of 2.  A growth norm_factor / norm_matrix above
 * about 1 / (b eps), b the half bandwidth, means that sigma sits on an eigenvalue of a leading sub-pencil (in factor order):
 * move the shift.  SLOD_ERR_ARGUMENT: NULL factor or out, member < 0 or >= the factor's members, a Cholesky factor. */
int slod_lod_factor_inertia(const slod_lod_factor *f, int member, slod_lod_factor_inertia_info *out);
/* The recursions of slod_lod_theta_steps, slod_lod_newmark_accel and slod_lod_newmark_steps (above, the same elementwise,
 * product and energy kernels) with the solve of a step done by slod_lod_factor_solve on a factor the caller built:
 *   slod_lod_theta_steps_direct    f_S factors  S = slod_lod_matrix_combine(1, M, theta dt, A)
 *   slod_lod_newmark_accel_direct  f_M factors  M
 *   slod_lod_newmark_steps_direct  f_S factors  S = slod_lod_matrix_combine(1 + gamma dt damp_mass, M,
 *                                                                          beta dt^2 + gamma dt damp_stiff, A)
 * with A the symmetrised stiffness; that the factor belongs to these coefficients is not checked.  One factor serves
 * any number of calls with the same dt and parameters.  There is no tolerance and no iteration count; nothing is read
 * back per step: the loop is queued on the handle's stream and waited for once, the energies are copied once at the
 * end.  A column's bits depend only on the factor, the matrices, the parameters and that column's state and loads, and
 * one call with n_steps = 2 equals two calls with n_steps = 1.  Return SLOD_OK or a negative slod_status.
 * SLOD_ERR_ARGUMENT: as the call without _direct, less rel_tol / max_iterations; a NULL factor; the factor of another
 * handle or row count.  Run on the handle's stream; synchronise.  The two steppers take a record armed by
 * slod_lod_time_record_arm (below), its launches inside the one queue-and-wait; slod_lod_newmark_accel_direct leaves it. */
int slod_lod_theta_steps_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const uint32_t *d_cols,
                                double dt, double theta, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                                const double *d_load, size_t ld_load, size_t load_step_stride);
int slod_lod_newmark_accel_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, const double *d_mass,
                                  const uint32_t *d_cols, double damp_mass, double damp_stiff, int n_rhs,
                                  const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                                  const double *d_load /* b^0, NULL = 0 */, size_t ld_load, double *d_a, size_t ld_a);
int slod_lod_newmark_steps_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const double *d_mass,
                                  const uint32_t *d_cols, double dt, double beta, double gamma, double damp_mass,
                                  double damp_stiff, int n_steps, int n_rhs, double *d_u, size_t ld_u, double *d_v, size_t ld_v,
                                  double *d_a, size_t ld_a, const double *d_load, size_t ld_load, size_t load_step_stride,
                                  double *kinetic   /* HOST [(n_steps + 1) * n_rhs], may be NULL */,
                                  double *potential /* HOST [(n_steps + 1) * n_rhs], may be NULL */);

/* ---- the LOD systems of a coefficient ensemble, one call per step for all members --------------
 * A handle with n_problems = K builds the bases of K coefficient realisations in one plan; these calls carry the
 * ensemble through the LOD space: K matrices, K loads, K solves, K reconstructions, then mean and variance (the
 * reference solves one problem, LOD.cc:976-1002).  The members share the grid, hence d_cols; they share no value.
 * Layouts:
 *   ensemble slab     member k in the single-problem slab layout at d_basis + k * member_stride (doubles), the same
 *                     for d_premult; member_stride = num_patches * stride is what a plan over the gids
 *                     0 .. K * num_patches - 1 with NULL offsets writes.
 *   ensemble matrix   one d_cols, word for word what slod_lod_matrix writes for rows 0 .. num_patches-1.  Values
 *                     member-minor: entry e of the single-matrix values array (e = (p * cap + j) * s * s + d * s + e')
 *                     of member k at d_values[e * ld_m + k], ld_m >= n_members, so that the lanes of a wave, which
 *                     hold consecutive members, read consecutive words.  n_members = 1, ld_m = 1 is the layout of
 *                     slod_lod_matrix; a member sub-range of a wider array is base + first member.
 *   coarse vectors    the coarse multi-vectors of the _multi calls, column k = member k (entry (i, k) at
 *                     base[i * ld + k]); fine fields field-major, member k at base + k * ld_fine.
 * Entries k >= n_members inside an ld are never read or written.  Every result of member k has the bits of the
 * single-problem call on member k's slab, matrix and vectors: the kernels are the same bodies and the same summation
 * orders with the member on a grid axis, and nothing depends on n_members, an ld, the member's position or the other
 * members.  Argument checks come before any device work (SLOD_ERR_ARGUMENT, with the call's name in slod_last_error):
 * NULL handle or array; n_members < 1 or > 65535; an ld below n_members; member_stride < num_patches * stride when
 * n_members > 1; and what a call lists.  SLOD_ERR_DEVICE without a usable GPU. */
/* Block rows of all num_patches patches for every member: member k's values are those of slod_lod_matrix with rows
 * 0 .. num_patches-1 on its slab, bit for bit.  d_cols is written once.  No row list is uploaded: fully ASYNCHRONOUS on
 * hip_stream (unlike slod_lod_matrix, which synchronises). */
int slod_lod_matrix_ensemble(slod_handle *h, const double *d_basis, const double *d_premult, size_t stride,
                             size_t member_stride, int n_members, double *d_values, size_t ld_m, uint32_t *d_cols,
                             void *hip_stream);
/* d_out[(p * s + d) * ld_out + k] = sum_i phi^(k)_{p,d}(i) f_k(i)  (slod_lod_rhs on member k's slab, bit for bit).
 * f_k = d_fine_rhs + k * ld_fine; ld_fine = 0: one load shared by all members; SLOD_ERR_ARGUMENT if ld_fine is neither 0
 * nor at least (NE+1)^2 * s.  Asynchronous on hip_stream. */
int slod_lod_rhs_ensemble(slod_handle *h, const double *d_basis, size_t stride, size_t member_stride, int n_members,
                          const double *d_fine_rhs, size_t ld_fine, double *d_out, size_t ld_out, void *hip_stream);
/* Y_k = A_k X_k: the fma chain of slod_lod_apply_multi over the slots of a row in ascending order, with member k's
 * matrix (the same bits).  SLOD_ERR_ARGUMENT also for d_x == d_y.  Asynchronous on hip_stream. */
int slod_lod_apply_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols,
                            const double *d_x, size_t ld_x, int n_members, double *d_y, size_t ld_y, void *hip_stream);
/* A_k u_k = rhs_k for every member: the recurrence of slod_lod_solve_multi (per-column scalars, freeze check every 8
 * iterations, fixed summation orders, no atomics) in which column k reads matrix k and the inverse diagonal of matrix k;
 * three launches per iteration for all members.  Column k of d_u, iterations[k] and rel_residual[k] are bit-identical
 * to slod_lod_solve_multi(n_rhs = 1) on member k's de-interleaved matrix and rhs.  Device workspace of
 * 5 * num_patches * s * n_members doubles, allocated per call.  Returns the largest per-member iteration count or a
 * negative slod_status; reaching max_iterations is not an error; SLOD_ERR_ARGUMENT also for max_iterations < 0.  Runs on
 * the handle's stream; synchronises. */
int slod_lod_solve_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols,
                            const double *d_rhs, size_t ld_rhs, int n_members, double *d_u, size_t ld_u,
                            double rel_tol, int max_iterations,
                            int *iterations /* HOST [n_members], may be NULL */,
                            double *rel_residual /* HOST [n_members], may be NULL */);
/* field k of d_fine = C_k u_k  (slod_lod_reconstruct on member k, bit for bit); ld_fine >= (NE+1)^2 * s.
 * Asynchronous on hip_stream. */
int slod_lod_reconstruct_ensemble(slod_handle *h, const double *d_basis, size_t stride, size_t member_stride,
                                  int n_members, const double *d_u, size_t ld_u, double *d_fine, size_t ld_fine,
                                  void *hip_stream);
/* Sample mean and unbiased variance over the members of the first `count` entries of n_members fields (field k at
 * d_fields + k * ld_fine, ld_fine >= count), per entry i:
 *   mean = (x_0 + x_1 + ..) / K  summed in ascending k;   var = sum_k (x_k - mean)^2 / (K - 1)  in ascending k,
 * difference, product and sum each rounded on its own (no fma): the bits of the obvious float64 loop.  K = 1: var = 0.
 * d_var may be NULL.  SLOD_ERR_ARGUMENT: NULL handle, d_fields or d_mean; n_members < 1; count = 0; ld_fine < count.
 * Asynchronous on hip_stream. */
int slod_ensemble_moments(slod_handle *h, const double *d_fields, size_t ld_fine, int n_members, size_t count,
                          double *d_mean, double *d_var /* may be NULL */, void *hip_stream);

/* ---- ensemble time stepping on banded Cholesky factors, one per member ---------------------------
 * The L2 side and the direct solver for a coefficient ensemble, in the layouts above: M_LOD of every member, the
 * symmetrised stiffness, S = M + theta dt A, one factor object that holds a factor per member, and the theta scheme on
 * it with one column per member.  The kernels are those of the single-problem calls (the row of slod_lod_mass_matrix,
 * the words of slod_lod_matrix_symmetrize and slod_lod_matrix_combine, the block column and the two sweeps of the
 * factor) with the member on a grid axis; a single-problem call is the instance n_members = 1, ld = 1.  Every result
 * of member k has the bits of the single-problem call on member k's de-interleaved data.  The common argument checks are
 * those of the ensemble block above.  Newmark on an ensemble factor is the block after this one, the eigensolver on an
 * ensemble factor the one after that.  Not built: a CG ensemble stepper, a partial refactor after slod_lod_matrix_update
 * (the stale factor serves as a preconditioner: slod_lod_solve_ensemble_precond), members spread over ranks, several columns
 * per member in a stepper. */
/* Block rows of M_LOD of all num_patches patches for every member: member k's values are those of slod_lod_mass_matrix
 * with rows 0 .. num_patches-1 on its slab, bit for bit.  d_cols is written once.  d_rho NULL: density 1; ld_rho = 0: one
 * density [NE][NE] shared by all members; else member k's density at d_rho + k * ld_rho.  SLOD_ERR_ARGUMENT also for a
 * d_rho with ld_rho neither 0 nor at least NE^2.  No row list is uploaded: ASYNCHRONOUS on hip_stream. */
int slod_lod_mass_matrix_ensemble(slod_handle *h, const double *d_basis, size_t stride, size_t member_stride, int n_members,
                                  const double *d_rho /* may be NULL */, size_t ld_rho, double *d_values, size_t ld_m,
                                  uint32_t *d_cols, void *hip_stream);
/* d_out = (A_k + A_k^T) / 2 per member, the bits of slod_lod_matrix_symmetrize.  SLOD_ERR_ARGUMENT also for
 * d_out == d_values.  Asynchronous on hip_stream. */
int slod_lod_matrix_symmetrize_ensemble(slod_handle *h, const double *d_values, size_t ld_in, const uint32_t *d_cols,
                                        int n_members, double *d_out, size_t ld_out, void *hip_stream);
/* d_out = alpha a + beta b per entry and member, (alpha a) + (beta b) rounded as in slod_lod_matrix_combine.  d_out may be
 * d_a or d_b when the leading dimensions of the two are equal; SLOD_ERR_ARGUMENT otherwise.  Asynchronous on hip_stream. */
int slod_lod_matrix_combine_ensemble(slod_handle *h, double alpha, const double *d_a, size_t ld_a, double beta,
                                     const double *d_b, size_t ld_b, int n_members, double *d_out, size_t ld_out,
                                     void *hip_stream);
/* slod_lod_factor_create for every member of an ensemble matrix: one allocation of n_members copies of the single
 * factor's storage (band tiles, diagonal tiles, pivots, reciprocal diagonal) and one row map; nb launches, each with the
 * block rows of a block column on blockIdx.x and the member on blockIdx.y.  Member k reads and writes its own copy and its
 * own status word only: a member that fails skips its later columns, the others finish, and member k's factor has the
 * bits of slod_lod_factor_create on member k's de-interleaved matrix.  One read-back at the end.  bad_pivot[k]: the
 * index of member k's first pivot that is not > 0, or -1; filled on SLOD_OK and on SLOD_ERR_NUMERIC.
 * SLOD_ERR_NUMERIC: a member failed; *out stays NULL, nothing stays allocated, slod_last_error names the call, the lowest
 * failing member, its pivot index and its value; the caller drops the members listed in bad_pivot and calls again.
 * SLOD_ERR_ARGUMENT (before any device work): NULL handle, array or out; n_members < 1 or > 65535; ld_m < n_members.
 * SLOD_ERR_DEVICE without a usable GPU.  Runs on the handle's stream; synchronises. */
int slod_lod_factor_create_ensemble(slod_handle *h, const double *d_values, size_t ld_m, int n_members,
                                    const uint32_t *d_cols, int32_t *bad_pivot /* HOST [n_members], may be NULL */,
                                    slod_lod_factor **out);
/* slod_lod_factor_get_info with the pivot range of one member (bytes: the whole allocation); slod_lod_factor_get_info
 * itself reports the range over all members.  A factor of slod_lod_factor_create has the one member 0.
 * SLOD_ERR_ARGUMENT: NULL factor or info, member < 0 or >= the factor's members. */
int slod_lod_factor_get_info_member(const slod_lod_factor *f, int member, slod_lod_factor_info *info);
/* Member first_member + k, k = 0 .. n_members-1, solves the n_rhs columns k * n_rhs .. k * n_rhs + n_rhs - 1 of d_rhs
 * into the same columns of d_u; with n_rhs = 1 column k is member k, the layout of the other ensemble calls.  One block
 * per 16 columns of a member and per member: the sweeps of slod_lod_factor_solve on that member's factor, so the bits of
 * a column depend only on its member's factor and that column.  d_u == d_rhs is allowed.  Asynchronous on hip_stream;
 * allocates nothing and reads nothing back.  slod_lod_factor_solve on a factor of more than one member is refused
 * (SLOD_ERR_ARGUMENT), as are the time loops of one matrix (slod_lod_theta_steps_direct, slod_lod_newmark_*_direct).
 * SLOD_ERR_ARGUMENT: NULL factor or array; n_rhs < 1; n_members < 1; first_member < 0 or first_member + n_members beyond
 * the factor's members; an ld below n_members * n_rhs. */
int slod_lod_factor_solve_ensemble(slod_lod_factor *f, int first_member, int n_members, const double *d_rhs, size_t ld_rhs,
                                   int n_rhs, double *d_u, size_t ld_u, void *hip_stream);
/* ---- CG preconditioned by a banded factor, stale or shared --------------------------------------
 * A u_c = rhs_c by the recurrence of slod_lod_solve_multi with  z = P^-1 r  (the two sweeps of slod_lod_factor_solve on
 * f_P, out of place) where that one has  z = D^-1 r.  f_P factors a matrix NEAR the one solved: the matrix before
 * slod_lod_matrix_update changed a few block rows (P^-1 A is then the identity plus a perturbation whose rank is bounded
 * by the rows that changed, and in exact arithmetic the iteration ends after rank + 1 steps whatever the contrast), one
 * member of an ensemble for all members, the step matrix of another dt, or the matrix itself (iterative refinement: one
 * or two iterations).  The reference has no counterpart (LOD.cc:990-998 runs CG + SSOR once).
 * Every column starts from u = 0 and has scalars of its own; five launches per iteration for all columns.  The stop rule
 * runs on the device in EVERY iteration: a column with r.r <= rel_tol^2 ||rhs_c||^2 (the recursive residual) is frozen
 * and never written again, any other column counts the iteration; iterations[c] is that device counter.  The host reads
 * the active words back every 4 iterations only to decide whether to go on launching: no output depends on that.  A zero
 * column gives u = 0, 0 iterations, residual 0.  Returns the largest per-column count or a negative slod_status; reaching
 * max_iterations is not an error.  iterations[c] and rel_residual[c] = ||r_c|| / ||rhs_c|| are HOST arrays (either may be
 * NULL), filled on SLOD_ERR_NUMERIC too.
 * f_P: a Cholesky factor, or an LDL^T factor all of whose pivots are positive (min_pivot > 0); any other LDL^T factor is
 * refused, SLOD_ERR_ARGUMENT "<call>: the preconditioner must be positive definite ..".  slod_lod_solve_multi_precond
 * takes a factor of one member and applies it to all columns.  slod_lod_solve_ensemble_precond (column k reads matrix k of
 * the ensemble matrix d_values, ld_m apart) takes a factor of one member, shared by all members, or a factor of exactly
 * n_members members, member k preconditioning column k; any other member count, a factor of another handle or row count
 * and a NULL factor are refused in the words of the calls on a factor above.  The factor is checked last and only read.
 * SLOD_ERR_NUMERIC: an active column met a p.Ap that is not > 0 (an indefinite matrix, NaN in the matrix) or an r.r that
 * is not finite.  That column sets its status and freezes where it stands, the other columns finish, and slod_last_error
 * reads "<call>: column c, iteration i: p.Ap = v is not > 0 .." ("member k" in the ensemble call) for the lowest such
 * column.  The handle and the factor stay usable.  A p.Ap that underflows to exactly 0 on a column about to converge
 * (rel_tol near 0) is reported the same way, where slod_lod_solve_multi takes a zero step: ask for no more than the
 * arithmetic can give.
 * Every sum has a fixed order (no atomics, no grid barrier): the bits of column c of d_u, iterations[c] and
 * rel_residual[c] depend only on the column's matrix, the column's factor member and column c of d_rhs -- not on n_rhs,
 * the column's position, an ld, the other columns, the read-back interval or the run.  Column k of the ensemble call
 * equals slod_lod_solve_multi_precond(n_rhs = 1) on member k's de-interleaved matrix with the single factor of member k's
 * preconditioner, as 64-bit words.  Entries c >= n_rhs of a row's ld are never read or written.  Device workspace of
 * 4 * num_patches * s * n_rhs doubles and the partial sums, one allocation per call.  Runs on the handle's stream;
 * synchronises.  SLOD_ERR_ARGUMENT (before any device work): NULL handle, array or factor; n_rhs / n_members < 1;
 * max_iterations < 0; an ld below the column count.  SLOD_ERR_DEVICE without a usable GPU.
 * Not built: a partial refactor of the band from the first dirty block column, this solve inside the time loops and the
 * eigensolvers, warm starts, a block-Krylov method. */
int slod_lod_solve_multi_precond(slod_handle *h, slod_lod_factor *f_P,
                                 const double *d_values, const uint32_t *d_cols,
                                 const double *d_rhs, size_t ld_rhs, int n_rhs, double *d_u, size_t ld_u,
                                 double rel_tol, int max_iterations,
                                 int *iterations /* HOST [n_rhs], may be NULL */,
                                 double *rel_residual /* HOST [n_rhs], may be NULL */);
int slod_lod_solve_ensemble_precond(slod_handle *h, slod_lod_factor *f_P,
                                    const double *d_values, size_t ld_m, const uint32_t *d_cols,
                                    const double *d_rhs, size_t ld_rhs, int n_members, double *d_u, size_t ld_u,
                                    double rel_tol, int max_iterations,
                                    int *iterations /* HOST [n_members], may be NULL */,
                                    double *rel_residual /* HOST [n_members], may be NULL */);
/* The loop of slod_lod_theta_steps_direct with one column per member: column k is advanced with matrix k of the ensemble
 * matrix d_stiffness (slod_lod_apply_ensemble) and member k of f_S, which factors
 * slod_lod_matrix_combine_ensemble(1, M, theta dt, A).  The loop is queued on the handle's stream and waited for once.
 * Column k has the bits of slod_lod_theta_steps_direct(n_rhs = 1) on member k's single factor and matrix; n_steps = 2
 * equals two calls with n_steps = 1.  Loads as in slod_lod_theta_steps (d_load NULL: none), column k = member k.
 * SLOD_ERR_ARGUMENT: NULL handle, matrix, d_cols or d_u; dt <= 0; theta outside [0, 1]; n_steps < 1; n_members < 1 or
 * > 65535; ld_m, ld_u or (with a load) ld_load below n_members; a NULL factor, the factor of another handle or row count,
 * a factor whose member count is not n_members.  A record armed by slod_lod_time_record_arm (below) is taken by this
 * call; its receivers hold n_members members and trace column m is member m's. */
int slod_lod_theta_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_m,
                                         const uint32_t *d_cols, double dt, double theta, int n_steps, int n_members,
                                         double *d_u, size_t ld_u, const double *d_load, size_t ld_load,
                                         size_t load_step_stride);

/* ---- the wave equation on a coefficient ensemble: Newmark on a factor per member -----------------
 * The second-order time stepper for  M_k u_k'' + C_k u_k' + A_k u_k = b_k(t),  C_k = damp_mass M_k + damp_stiff A_k, with
 * member k of an ensemble in column k: the recursions of slod_lod_newmark_accel_direct and slod_lod_newmark_steps_direct
 * in which column k reads member k of the ensemble matrices d_stiffness (leading dimension ld_a_m) and d_mass (ld_m_m;
 * the two may differ) and is solved on member k of the factor.  The product and energy kernels are those of the single
 * calls with a matrix per column (the chain of slod_lod_apply_ensemble); predictor, corrector, the sums of the energies
 * and the sweeps of the factor are the same launches.  Column k of every result has the bits of the single-problem call
 * with n_rhs = 1 on member k's de-interleaved matrices, single factor, state and loads; nothing depends on n_members, an
 * ld, the member's position or the other members; entries k >= n_members inside an ld are never read or written.
 * Argument checks come before any device work (SLOD_ERR_ARGUMENT, the call's name in slod_last_error): what the single
 * call refuses, and n_members < 1 or > 65535, a matrix or vector ld below n_members (ld_load only with a load), a NULL
 * factor, the factor of another handle or row count, a factor whose member count is not n_members (checked last).
 * slod_lod_newmark_*_direct on a factor of several members stays refused.  Not built: these loops on CG, several columns
 * per member. */
/* out[k] = x_k^T (A_k y_k): slod_lod_inner_multi with member k's matrix, the same bits (the fma chain over the slots,
 * the product with x rounded on its own, 16 rows into a partial, the partials in ascending group order).  d_x == d_y
 * gives the quadratic form.  A member sub-range is d_values + first member with the vectors' base moved alike.
 * Synchronises hip_stream. */
int slod_lod_inner_ensemble(slod_handle *h, const double *d_values, size_t ld_m, const uint32_t *d_cols, const double *d_x,
                            size_t ld_x, const double *d_y, size_t ld_y, int n_members,
                            double *out /* HOST [n_members] */, void *hip_stream);
/* M_k a_k = b^0_k - A_k (u_k + damp_stiff v_k) - damp_mass M_k v_k on member k of f_M, which factors the ensemble matrix
 * d_mass.  d_load NULL: b^0 = 0.  With damp_mass = 0 the mass product is skipped and d_mass is not read.  u and v are read
 * only.  Runs on the handle's stream; synchronises. */
int slod_lod_newmark_accel_ensemble_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, size_t ld_a_m,
                                           const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, double damp_mass,
                                           double damp_stiff, int n_members, const double *d_u, size_t ld_u,
                                           const double *d_v, size_t ld_v, const double *d_load /* b^0, NULL = 0 */,
                                           size_t ld_load, double *d_a, size_t ld_a);
/* The loop of slod_lod_newmark_steps_direct, one column per member, on member k of f_S, which factors
 *   slod_lod_matrix_combine_ensemble(1 + gamma dt damp_mass, M, beta dt^2 + gamma dt damp_stiff, A)
 * with A the symmetrised ensemble stiffness; that the factor belongs to these coefficients is not checked.  Loads as in
 * slod_lod_newmark_steps, column k = member k.  kinetic / potential: entry [step * n_members + k], both or neither; with
 * both NULL and damp_mass = 0 d_mass is not read.  The loop is queued on the handle's stream and waited for once, the
 * energies stay on the device and are copied once at the end; device workspace (2 vectors of n_members columns, the
 * partials and the energies) is allocated once per call.  n_steps = 2 equals two calls with n_steps = 1 carrying u, v, a
 * over.  A record armed by slod_lod_time_record_arm (below) is taken by this call (u and / or v of n_members members);
 * slod_lod_newmark_accel_ensemble_direct leaves it. */
int slod_lod_newmark_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, size_t ld_a_m,
                                           const double *d_mass, size_t ld_m_m, const uint32_t *d_cols, double dt,
                                           double beta, double gamma, double damp_mass, double damp_stiff, int n_steps,
                                           int n_members, double *d_u, size_t ld_u, double *d_v, size_t ld_v, double *d_a,
                                           size_t ld_a, const double *d_load, size_t ld_load, size_t load_step_stride,
                                           double *kinetic   /* HOST [(n_steps + 1) * n_members], may be NULL */,
                                           double *potential /* HOST [(n_steps + 1) * n_members], may be NULL */);

/* ---- eigenpairs on banded Cholesky factors, for one pencil and per ensemble member ----------------
 * slod_lod_eigs with the inner CG replaced by the two sweeps of a factor: no inner tolerance, no inner iteration count.
 * f_S factors a symmetric positive definite  S = A - sigma M  with sigma < lambda_1, built by the caller from
 * slod_lod_matrix_combine(1, sym A, -sigma, M) (or its _ensemble form) and slod_lod_factor_create(_ensemble); sigma = 0
 * means the factor of sym(A).  The eigensolver never sees sigma: Rayleigh-Ritz is done on the pencil (A, M) itself, so
 * eigenvalues and residuals are those of (A, M) whatever the shift.
 *   - That S belongs to these matrices is NOT checked, as in the time steppers on a factor.
 *   - sigma < lambda_1 is the caller's duty: slod_lod_factor_create* answers SLOD_ERR_NUMERIC for an S that is not
 *     positive definite, so a factor that exists is one of a definite S.
 *   - Column j contracts by about (lambda_j - sigma) / (lambda_{m+1} - sigma) per outer iteration, m = n_block.
 * Outer iteration k = 1, 2, ..:  Y = M X;  S Z = Y on the factor;  W = A Z, V = M Z;  Ga = sym(Z^T W), Gm = sym(Z^T V);
 * the Ritz step;  X = Z Q;  res_j as documented for slod_lod_eigs;  stop when res_j <= tol for all j < n_eig or at
 * k = max_outer (not an error).  The Gram, Ritz, rotate and residual kernels are those of slod_lod_eigs; the products run
 * the fma chain of slod_lod_apply_multi.  An LDL^T factor (slod_lod_factor_create_ldl) is taken as well.  Not built: LOBPCG,
 * locking of converged columns, n_block > 64. */
/* One pencil.  Arguments as in slod_lod_eigs, less the inner parameters.  Returns the number of outer iterations run
 * (>= 1) or a negative slod_status.  SLOD_ERR_NUMERIC: rank-deficient block as in slod_lod_eigs; d_x then holds the block
 * the failed iteration started from, eigenvalues and residuals those of the last completed iteration (0 if none).
 * Fixed summation orders: the same inputs give the same bits, run after run.  This is the one-member instance of the
 * ensemble call below (n_members = 1, ld = 1).
 * SLOD_ERR_ARGUMENT (before any device work, the call's name in slod_last_error): NULL handle, matrix, d_cols, d_x,
 * eigenvalues or residuals; n_eig < 1; n_block < n_eig; n_block > 64 or > num_patches * s; start not 0 or 1; tol <= 0 or
 * NaN; max_outer < 1; ld_x < n_block; a NULL factor, the factor of another handle or row count, a factor of more than
 * one member (checked last).  Runs on the handle's stream; synchronises. */
int slod_lod_eigs_direct(slod_handle *h, slod_lod_factor *f_S,
                         const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                         int n_eig, int n_block, int start, double *d_x, size_t ld_x,
                         double tol, int max_outer,
                         double *eigenvalues /* HOST [n_block] */,
                         double *residuals   /* HOST [n_block] */);
/* The n_members pencils (A_k, M_k) of a coefficient ensemble at once, member k on member k of f_S.  Layout of
 * slod_lod_factor_solve_ensemble: member k owns columns k * n_block .. k * n_block + n_block - 1 of d_x,
 * ld_x >= n_members * n_block, entries beyond that are never read or written; the matrices are member-minor on one
 * pattern (ld_a_m, ld_m_m >= n_members, the two may differ).  start = 0 writes the sine block of slod_lod_eigs into every
 * member's columns; start = 1 takes the caller's block.  HOST eigenvalues and residuals: entry [k * n_block + j].
 * Every member stops on its own, on the device: the residual kernel compares member k's residuals with tol (the <= of
 * slod_lod_eigs) and sets its done word when all j < n_eig pass, or when its Ritz step failed; from then on the Ritz,
 * rotate and residual kernels skip that member, whose X, theta and residuals stay those of its last iteration (the factor
 * solve and the products go on running on its frozen columns).  The host reads theta, residuals, status and done of all
 * members in one copy per outer iteration and stops when every member is done, or at max_outer.
 * member_status[k]: the outer iterations member k ran (>= 1), or SLOD_ERR_NUMERIC for a rank-deficient block; member k's
 * columns of d_x then hold the block its failed iteration started from, its eigenvalues and residuals those of its last
 * completed iteration (0 if none), and the other members finish and are valid.
 * Returns the largest count if every member succeeded; SLOD_ERR_NUMERIC if a member failed (slod_last_error names the
 * call, the lowest failing member, its column and its outer iteration); else a negative slod_status.
 * Member k's X, eigenvalues, residuals and count have the bits of slod_lod_eigs_direct on member k's de-interleaved
 * matrices, its single factor and its own start block: nothing depends on n_members, an ld, the member's position or the
 * other members.  Device workspace (4 vectors of n_members * n_block columns, per member the slab partials, Ga, Gm, Q)
 * allocated once per call.
 * SLOD_ERR_ARGUMENT (before any device work, the call's name in slod_last_error): what slod_lod_eigs_direct refuses, and
 * n_members < 1 or > 65535; ld_a_m or ld_m_m < n_members; ld_x < n_members * n_block; NULL member_status; a factor whose
 * member count is not n_members (checked last).  Runs on the handle's stream; synchronises. */
int slod_lod_eigs_ensemble_direct(slod_handle *h, slod_lod_factor *f_S,
                                  const double *d_stiffness, size_t ld_a_m, const double *d_mass, size_t ld_m_m,
                                  const uint32_t *d_cols, int n_members, int n_eig, int n_block, int start,
                                  double *d_x, size_t ld_x, double tol, int max_outer,
                                  double *eigenvalues   /* HOST [n_members * n_block] */,
                                  double *residuals     /* HOST [n_members * n_block] */,
                                  int    *member_status /* HOST [n_members] */);
/* ---- eigenpairs nearest an interior shift --------------------------------------------------------
 * slod_lod_eigs_direct / slod_lod_eigs_ensemble_direct with one more argument, sigma, which may lie anywhere outside the
 * spectrum's points: f_S factors  S = sym(A) - sigma M  (slod_lod_factor_create_ldl(_ensemble); a Cholesky factor is taken
 * too when S is definite).  The outer iteration, the Gram, rotate and residual kernels, the done words, the read-backs and
 * member_status are those calls'; after the Ritz step the columns are ordered by |theta_j - sigma| ascending, ties by
 * ascending theta_j, then by index.  So columns j < n_eig hold the pairs NEAREST sigma, they are the ones tested against
 * tol, and the guard columns are the ones farthest from sigma.  Column j contracts by about
 * |lambda_(j) - sigma| / |lambda_(m+1) - sigma| per outer iteration, the eigenvalues taken in order of distance from sigma.
 * That the number of eigenvalues below sigma is slod_lod_factor_inertia's n_negative lets a caller check that none was
 * missed.  The ensemble form takes one sigma for all members.
 * start = 1 takes the caller's block.  start = 0 writes a hashed block (the sine block of slod_lod_eigs starts in the lowest
 * modes, the wrong end for an interior shift), the same for every member: entry (caller's row i = p s + d, column j) is
 *   z = ((uint64) i << 32 | j) + 0x9E3779B97F4A7C15;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;   z = (z ^ z >> 27) * 0x94D049BB133111EB;   z ^= z >> 31;
 *   x = (double) (z >> 11) * 2^-52 - 1        (all in uint64 arithmetic, x in [-1, 1))
 * SLOD_ERR_ARGUMENT: what the _direct calls refuse, and sigma NaN or infinite (checked before the factor). */
int slod_lod_eigs_shift_direct(slod_handle *h, slod_lod_factor *f_S, double sigma,
                               const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                               int n_eig, int n_block, int start, double *d_x, size_t ld_x,
                               double tol, int max_outer,
                               double *eigenvalues /* HOST [n_block] */,
                               double *residuals   /* HOST [n_block] */);
int slod_lod_eigs_shift_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, double sigma,
                                        const double *d_stiffness, size_t ld_a_m, const double *d_mass, size_t ld_m_m,
                                        const uint32_t *d_cols, int n_members, int n_eig, int n_block, int start,
                                        double *d_x, size_t ld_x, double tol, int max_outer,
                                        double *eigenvalues   /* HOST [n_members * n_block] */,
                                        double *residuals     /* HOST [n_members * n_block] */,
                                        int    *member_status /* HOST [n_members] */);

/* ---- the frequency response: complex symmetric banded LDL^T, a sweep of frequencies per call --------
 * The steady response to a harmonic load: for  M u'' + C u' + A u = Re(b e^{i omega t})  with the Rayleigh damping of the
 * Newmark calls, C = damp_mass M + damp_stiff A, the amplitude u solves
 *   S(omega) u = b,   S(omega) = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M,
 * complex SYMMETRIC (not Hermitian).  The third kind of factor is  S = L D L^T  with the plain transpose, complex 1 x 1
 * pivots and no pivoting, in the tiles, the ordering, the row map and the padding of the real factors, every array in two
 * planes (real, imaginary).  For omega > 0 and any positive damping the imaginary part of S is positive definite, so
 * z^H S_k z has a non-zero imaginary part for every leading block S_k and z != 0: every leading block is non-singular and
 * the factorisation exists without a permutation.  Its stability is measured, as for the real LDL^T: the growth
 * || |L| |D| |L^T| ||_inf / ||S||_inf (moduli) is reported, and slod_lod_harmonic_response returns the true residual.
 *
 * slod_lod_factor_create_zldl factors the n_members matrices  S_k = alpha_k A + beta_k B  in one object, members as in
 * slod_lod_factor_create_ensemble (at most 65535, one allocation): a frequency sweep is n_members pairs (alpha, beta) on
 * one pair (A, B) = (sym(A_LOD), M_LOD).  The K matrices are never built: the band is filled with
 *   re = (alpha_re a) + (beta_re b),   im = (alpha_im a) + (beta_im b),
 * every product and every sum rounded on its own.  Member k's factor has the same words whatever n_members and its
 * position are.  SLOD_ERR_NUMERIC: a pivot has both parts zero or a part that is infinite or NaN; slod_last_error reads
 *   "slod_lod_factor_create_zldl: member k: pivot r of n is zero or not finite (re, im)",
 * bad_pivot[k] is the first such pivot of member k (-1: none), *out stays NULL and nothing stays allocated.
 * SLOD_ERR_ARGUMENT, before any device work: NULL handle, array, alpha, beta or out; n_members < 1 or > 65535; a NaN or
 * infinite coefficient.
 * On a complex factor slod_lod_factor_get_info(_member) reports min_pivot / max_pivot as the range of |D|, and
 * slod_lod_factor_inertia fills min_abs_pivot / max_abs_pivot and the two norms (of moduli) and sets
 * n_negative = n_positive = -1: a complex D has no signs.
 *
 * slod_lod_factor_solve_complex: L y = b, L^T x = D^-1 y on complex tiles, with the deal of tiles to waves and the order
 * of summation of slod_lod_factor_solve.  The bits of a column of u depend only on its member's factor and on that column
 * of the rhs: not on n_rhs, a leading dimension, the column's position, shared_rhs, the other members or the run.  In
 * place (d_u_re == d_rhs_re, d_u_im == d_rhs_im) is allowed unless shared_rhs is set with more than one member.
 * SLOD_ERR_ARGUMENT: NULL factor or array (d_rhs_im may be NULL); n_rhs < 1 or n_members < 1; a real factor; members
 * outside the factor; ld_u < n_members n_rhs; ld_rhs < n_rhs (shared) or < n_members n_rhs; that in-place case.
 *
 * Every other call that takes a factor refuses a complex one (slod_lod_factor_solve(_ensemble), the theta and Newmark
 * _direct calls, the slod_lod_eigs*_direct calls, the _precond calls): SLOD_ERR_ARGUMENT,
 *   "<call>: a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex".
 * (The implicit Runge-Kutta steppers slod_lod_irk_*_steps_direct, below, are the time loops on a complex factor.)
 *
 * S_k = alpha_k A + beta_k B, complex alpha_k, beta_k; A, B: values arrays of two full sets of block rows on one d_cols
 * (sym(A_LOD), M_LOD); ONLY THE LOWER TRIANGLE IN FACTOR ORDER IS READ.  alpha, beta: HOST [n_members][2] (re, im). */
int slod_lod_factor_create_zldl(slod_handle *h, const double *d_a, const double *d_b, const uint32_t *d_cols,
                                const double *alpha, const double *beta, int n_members,
                                int32_t *bad_pivot /* HOST [n_members], may be NULL */, slod_lod_factor **out);
/* member first_member + k solves columns k n_rhs .. k n_rhs + n_rhs - 1 (layout of slod_lod_factor_solve_ensemble) of
 * (d_u_re, d_u_im).  shared_rhs != 0: every member reads columns 0 .. n_rhs-1 of the rhs (ld_rhs >= n_rhs).
 * d_rhs_im NULL = 0.  Asynchronous, allocates nothing, reads nothing back. */
int slod_lod_factor_solve_complex(slod_lod_factor *f, int first_member, int n_members, const double *d_rhs_re,
                                  const double *d_rhs_im, size_t ld_rhs, int n_rhs, int shared_rhs,
                                  double *d_u_re, double *d_u_im, size_t ld_u, void *hip_stream);
/* The sweep in one call: frequency k is the member with  alpha_k = (1, omega_k damp_stiff),
 * beta_k = (-(omega_k omega_k), omega_k damp_mass)  (one rounding each), solved on the load, which all frequencies share,
 * into the columns k n_rhs .. k n_rhs + n_rhs - 1 of (d_u_re, d_u_im): the words of slod_lod_factor_create_zldl +
 * slod_lod_factor_solve_complex on these coefficients.  d_stiffness is the symmetrised stiffness.  The call factors and
 * solves in chunks of at most 64 frequencies, which bounds the memory (one factor allocation per chunk); a chunk is queued
 * whole on the handle's stream and waited for once, and the result does not depend on the chunking.
 * rel_residual[k n_rhs + c] = ||b_c - S(omega_k) u||_2 / ||b_c||_2, formed after the solve from the matrices themselves,
 * not from the factor: the four products A u_re, A u_im, M u_re, M u_im by the fma chain of slod_lod_apply_multi, combined
 * with the complex coefficients per entry, fixed-order sums, no atomics.  A zero load column gives u = 0 and residual 0.
 * growth[k] = norm_factor / norm_matrix of member k (slod_lod_factor_inertia).
 * omega = 0, or no damping at all, is allowed: S is then real, the imaginary planes stay exact zeros, and the existence of
 * the factor is the caller's risk, as with slod_lod_factor_create_ldl.
 * Return SLOD_OK; SLOD_ERR_NUMERIC, "slod_lod_harmonic_response: frequency k: pivot r of n is zero or not finite (re, im)"
 * (the outputs are then undefined); or another negative slod_status.  SLOD_ERR_ARGUMENT, before any device work: a NULL
 * handle, matrix, d_cols, omega, d_load_re or u; negative, NaN or infinite damping; n_freq < 1 or n_rhs < 1; omega[k]
 * negative, NaN or infinite (or so large that omega^2 overflows); ld_load < n_rhs; ld_u < n_freq n_rhs.
 * Runs on the handle's stream and has finished when it returns.
 * Not built: coefficient ensembles x frequencies, 2 x 2 pivots, damping that is not Rayleigh, adaptive frequency
 * refinement, this factor as a preconditioner.  (Of these, coefficient ensembles x frequencies exist by now as a call of
 * their own: slod_lod_harmonic_response_ensemble, below.) */
int slod_lod_harmonic_response(slod_handle *h, const double *d_stiffness, const double *d_mass, const uint32_t *d_cols,
                               double damp_mass, double damp_stiff, const double *omega /* HOST [n_freq] */, int n_freq,
                               const double *d_load_re, const double *d_load_im /* NULL = 0 */, size_t ld_load, int n_rhs,
                               double *d_u_re, double *d_u_im, size_t ld_u,
                               double *rel_residual /* HOST [n_freq * n_rhs], may be NULL */,
                               double *growth       /* HOST [n_freq], may be NULL */);

/* ---- the frequency response of a coefficient ensemble: K members x F frequencies per call -----------
 * The calls above for the K members of a coefficient ensemble on one pattern (the ensemble matrix layout: entry e of
 * member m at values[e ld_m + m]).  The use is an uncertainty band around a transfer function: mean and spread of
 * ||u(omega)|| over the realisations.  The factor members are numbered flat, frequency-major and member-minor:
 *   factor member j = k K + m  is  S_j = alpha_k A_m + beta_k B_m,  coefficient pair (frequency) k on the matrices of member m.
 * The banded factor pays one launch per block column whatever the number of members on it, so K x F members in one object
 * cost the launches of one.
 *
 * LAYOUT of slod_lod_harmonic_response_ensemble: the response of (frequency k, member m, load column c) is column
 * (k K + m) n_rhs + c of (d_u_re, d_u_im), ld_u >= F K n_rhs.  Member m's loads are the columns m n_rhs + c of d_load,
 * ld_load >= K n_rhs; all frequencies share them.  With n_rhs = 1 the block of K columns at offset k K is therefore an
 * ensemble coarse multi-vector, column = member: slod_lod_rhs_ensemble (the loads differ per member because C^T f does),
 * slod_lod_reconstruct_ensemble, slod_lod_inner_ensemble and slod_ensemble_moments apply to a frequency's block as they
 * are, by pointer offset with ld = F K.
 * THE BITS: for every (k, m, c) the words of u, rel_residual and growth equal those of slod_lod_harmonic_response on
 * member m's de-interleaved matrices and load at the single frequency omega_k (coefficients formed as there); they do not
 * depend on K, F, a leading dimension, the member's position, the chunking or the run.  Padding entries >= K inside
 * ld_a_m / ld_m_m and columns beyond the last inside ld_u are never read or written.
 * The call works through the flat index j in chunks of at most 64 consecutive j (a chunk may start and end inside a
 * frequency): one factor allocation per chunk, every chunk queued whole on the handle's stream and waited for once.
 * n_freq n_members is unbounded there; slod_lod_factor_create_zldl_ensemble takes n_coef n_members <= 65535.
 * quantities[col] = (u^H M u, u^H A u, Re u^H b, Im u^H b), col = (k K + m) n_rhs + c, A the symmetrised stiffness as
 * passed: per row  u_re (M u)_re + u_im (M u)_im  (the same for A) and the two parts of conj(u_i) b_i  from the four
 * products of the residual step, every product and sum rounded on its own, the rows summed in the fixed order of the
 * residual, no atomics.  A zero load column gives four exact zeros.  Amplitude is sqrt(u^H M u), dissipated power
 * omega (damp_mass u^H M u + damp_stiff u^H A u) / 2, and the balance
 *   omega (damp_mass u^H M u + damp_stiff u^H A u) = Im u^H b
 * tells whether a response is to be trusted.
 * SLOD_ERR_NUMERIC reads
 *   "slod_lod_harmonic_response_ensemble: frequency k, member m: pivot r of n is zero or not finite (re, im)"
 * with the lowest flat j first; slod_lod_factor_create_zldl_ensemble names "coefficient k, member m", fills
 * bad_pivot[k K + m] with the single call's index for that matrix (-1 elsewhere), leaves *out NULL and nothing allocated.
 * SLOD_ERR_ARGUMENT, before any device work, with the call's name: what the single calls refuse; n_members < 1 or > 65535;
 * n_coef < 1 or n_coef n_members > 65535; ld_a_m, ld_b_m or ld_m_m below n_members; ld_load < n_members n_rhs;
 * ld_u / n_rhs < n_freq n_members; for the solve rhs_members < 1, members outside the factor, a real factor, a rhs
 * leading dimension below the columns read, and in place (d_u == d_rhs) whenever two of the call's factor members read
 * the same rhs columns or a member would read columns another one writes (first_member not a multiple of rhs_members).
 * On the factor object slod_lod_factor_get_info_member(f, j, ..) and slod_lod_factor_inertia(f, j, ..) take the flat j;
 * every real consumer refuses the object with the message above.
 * Not built: members or frequencies spread over ranks, 2 x 2 pivots, damping that is not Rayleigh, adaptive frequency
 * refinement, the complex factor as a preconditioner, output functionals other than u^H b, the deal.II adapter. */

/* Factor member j = k * n_members + m is  S_j = alpha_k A_m + beta_k B_m;  A, B ensemble matrices (values member-minor,
 * entry e of member m at d_a[e * ld_a_m + m]) on one d_cols; alpha, beta HOST [n_coef][2]. */
int slod_lod_factor_create_zldl_ensemble(slod_handle *h, const double *d_a, size_t ld_a_m, const double *d_b, size_t ld_b_m,
                                         int n_members, const uint32_t *d_cols, const double *alpha, const double *beta,
                                         int n_coef, int32_t *bad_pivot /* HOST [n_coef * n_members], may be NULL */,
                                         slod_lod_factor **out);

/* slod_lod_factor_solve_complex in which factor member j reads the rhs columns (j % rhs_members) * n_rhs .. + n_rhs - 1
 * and writes the columns (j - first_member) * n_rhs .. of u.  rhs_members = 1 is shared_rhs; rhs_members = the factor's
 * member count is the distinct case. */
int slod_lod_factor_solve_complex_ensemble(slod_lod_factor *f, int first_member, int n_members, const double *d_rhs_re,
                                           const double *d_rhs_im, size_t ld_rhs, int n_rhs, int rhs_members,
                                           double *d_u_re, double *d_u_im, size_t ld_u, void *hip_stream);

int slod_lod_harmonic_response_ensemble(slod_handle *h, const double *d_stiffness, size_t ld_a_m, const double *d_mass,
                                        size_t ld_m_m, const uint32_t *d_cols, int n_members, double damp_mass,
                                        double damp_stiff, const double *omega /* HOST [n_freq] */, int n_freq,
                                        const double *d_load_re, const double *d_load_im /* NULL = 0 */, size_t ld_load,
                                        int n_rhs, double *d_u_re, double *d_u_im, size_t ld_u,
                                        double *rel_residual /* HOST [n_freq*n_members*n_rhs], may be NULL */,
                                        double *growth       /* HOST [n_freq*n_members], may be NULL */,
                                        double *quantities   /* HOST [n_freq*n_members*n_rhs][4], may be NULL */);

/* ---- fourth-order time stepping: two-stage implicit Runge-Kutta on the complex factor ----------------
 * The direct steppers above are second order at best and pay one banded solve per step, whose cost is the serial walk of
 * the block rows, not the arithmetic.  A two-stage implicit Runge-Kutta scheme has a 2 x 2 Butcher matrix
 * A_rk = T diag(lambda, conj lambda) T^-1 with a complex conjugate pair of eigenvalues; for a linear system with real data
 * the two transformed stage equations are conjugates of each other, so ONE complex solve per step, on a member of a
 * factor of slod_lod_factor_create_zldl, gives
 *   SLOD_IRK_GAUSS2   Gauss-Legendre, order 4, A-stable, conserves the quadratic energy of the undamped wave equation;
 *                     lambda = 1/4 + i sqrt(3)/12, c = (1/2 - sqrt(3)/6, 1/2 + sqrt(3)/6)
 *   SLOD_IRK_RADAU2A  Radau IIA, order 3, L-stable (stiff modes are damped out, the scheme for heat flow);
 *                     lambda = 1/3 + i sqrt(2)/6, c = (1/3, 1).
 * With z = dt lambda, tau the first row of T^-1, sigma = tau_1 + tau_2, mu = b^T T[:,0] (host constants in long double)
 * and b_i the load at t_k + c_i dt:
 *   heat  M u' + A u = b(t):  S = M + z A;  r = tau_1 (b_1 - A u) + tau_2 (b_2 - A u);  S w = r;  u += 2 dt Re(mu w)
 *   wave  M u'' + C u' + A u = b(t), C = damp_mass M + damp_stiff A:  S = (1 + z damp_mass) M + (z damp_stiff + z^2) A;
 *         r = tau_1 b_1 + tau_2 b_2 - sigma [A (u + (z + damp_stiff) v) + damp_mass M v];  S w_v = r;
 *         w_u = sigma v + z w_v;  u += 2 dt Re(mu w_u);  v += 2 dt Re(mu w_v).   No acceleration vector is carried.
 * Re S is symmetric positive definite (Re lambda > 0, Re z^2 > 0), so every leading block of S is non-singular and the
 * factorisation exists without pivoting; its growth is measured, as for every complex factor (slod_lod_factor_inertia).
 *
 * slod_lod_irk_coefficients returns the pair for slod_lod_factor_create_zldl(h, sym(A_LOD), M_LOD, d_cols, alpha, beta, 1,
 * ..):  heat (order 1) alpha = z, beta = 1;  wave (order 2) alpha = z damp_stiff + z^2, beta = 1 + z damp_mass, formed in
 * long double and rounded once per part.  Host only, no handle; an error text is read by slod_last_error(NULL).
 * SLOD_ERR_ARGUMENT: NULL alpha or beta; an unknown scheme or order; dt <= 0, NaN or infinite; a negative, NaN or infinite
 * damping; a damping given with order = 1; a coefficient that overflows.
 *
 * THE STEPPERS run n_steps on d_u (and d_v) in place on member `member` of f_S, so one factor object may hold several dt.
 * d_stiffness is the symmetrised stiffness the factor was built from.  LOADS are given at the stage times: stage i
 * (0, 1) of step k is at d_load + (2 k + i) load_stage_stride; stride 0 is one constant load, d_load NULL the zero load.
 * kinetic, potential: HOST [(n_steps + 1) n_rhs] with the meaning and the sums of slod_lod_newmark_steps (1/2 v^T M v,
 * 1/2 u^T A u, row 0 the entry state); both NULL: not computed.  A step is three launches (right-hand side: the fma chains
 * of slod_lod_apply_multi per row on one read of the row's column indices, then the complex combination with every product
 * and sum rounded on its own; the sweeps of slod_lod_factor_solve_complex, out of place; the update) and two more with the
 * energies.  The loop is queued whole on the handle's stream and waited for once: no allocation inside the loop, nothing
 * read back per step; the mass product is skipped when damp_mass = 0.
 * THE BITS of a column depend only on the factor member, the matrices, the parameters and that column's state and loads:
 * not on n_rhs, a leading dimension, the column's position or the run; one call with n_steps = 2 equals two calls with
 * n_steps = 1.  That the factor belongs to dt, the scheme and the dampings is not checked, as for the other _direct calls.
 * SLOD_ERR_ARGUMENT, before any device work, with the call's name: a NULL handle, matrix, d_cols or state; an unknown
 * scheme; dt <= 0, NaN or infinite; a negative, NaN or infinite damping; n_steps < 1 or n_rhs < 1; a leading dimension
 * below n_rhs; exactly one of kinetic / potential; a NULL factor; the factor of another handle / row count; a real factor,
 *   "<call>: takes a complex factor (slod_lod_factor_create_zldl)";
 * a member outside the factor.  The real consumers go on refusing complex factors as above.
 * Not built: three-stage schemes (Radau IIA of order 5 and Gauss of order 6 need one real and one complex member),
 * CG or PCG as the stage solver, step-size control, dense output, the deal.II adapter.  (The ensemble forms are
 * slod_lod_irk_*_steps_ensemble_direct, below.)  The four steppers take a record armed by slod_lod_time_record_arm (below). */
enum slod_irk_scheme { SLOD_IRK_GAUSS2 = 0, SLOD_IRK_RADAU2A = 1 };
int slod_lod_irk_coefficients(int scheme, int order /* 1 heat, 2 wave */, double dt, double damp_mass, double damp_stiff,
                              double alpha[2], double beta[2]);
int slod_lod_irk_heat_steps_direct(slod_handle *h, slod_lod_factor *f_S, int member, int scheme, const double *d_stiffness,
                                   const uint32_t *d_cols, double dt, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                                   const double *d_load /* NULL = 0 */, size_t ld_load, size_t load_stage_stride);
int slod_lod_irk_wave_steps_direct(slod_handle *h, slod_lod_factor *f_S, int member, int scheme, const double *d_stiffness,
                                   const double *d_mass, const uint32_t *d_cols, double dt, double damp_mass, double damp_stiff,
                                   int n_steps, int n_rhs, double *d_u, size_t ld_u, double *d_v, size_t ld_v,
                                   const double *d_load /* NULL = 0 */, size_t ld_load, size_t load_stage_stride,
                                   double *kinetic   /* HOST [(n_steps+1)*n_rhs], may be NULL */,
                                   double *potential /* HOST [(n_steps+1)*n_rhs], may be NULL */);

/* ---- implicit Runge-Kutta time stepping for a coefficient ensemble: K members per call ----------------
 * The two steppers above with a matrix, a factor member and a column per member of a coefficient ensemble on one pattern
 * (the ensemble matrix layout: entry e of member m at values[e ld + m]).  The use is an uncertainty band on a transient
 * at fourth order: the serial walk of the band, which is the cost of a step, is shared by the K members of one launch.
 * LAYOUT, member = column as in slod_lod_newmark_steps_ensemble_direct: column m of d_u (and d_v) is member m's state; it
 * is advanced on factor member first_member + m with member m of d_stiffness (ld_a_m) and d_mass (ld_m_m).  For a factor
 * of slod_lod_factor_create_zldl_ensemble with n_coef pairs of slod_lod_irk_coefficients, first_member = k K picks dt_k,
 * so several dt x K members sit in one object; first_member need not be a multiple of n_members (a member sub-range is
 * first_member = k K + m0 with every pointer offset by m0 members), and factor member first_member + m always reads
 * column m of the right-hand side.
 * LOADS: stage i (0, 1) of step k, member m, row r at d_load[(2 k + i) load_stage_stride + r ld_load + m]; stride 0 is
 * one constant load, d_load NULL the zero load.  kinetic, potential: HOST [(n_steps + 1) n_members], per member
 * 1/2 v_m^T M_m v_m and 1/2 u_m^T A_m u_m with the sums of slod_lod_newmark_steps_ensemble_direct, row 0 the entry state.
 * A step is three launches, five with the energies, for any number of members: the right-hand side (the chains of the
 * single call on member m's words, the loads of 8 slots issued ahead of the first fma, every word of A read once for
 * A u and A v and the words of M in the same batch), the complex sweeps with a member per blockIdx.y, the update.  One
 * allocation per call, the loop queued whole on the handle's stream and waited for once, nothing read back per step.
 * THE BITS: column m's u, v, kinetic and potential are, as 64-bit words, those of slod_lod_irk_{heat,wave}_steps_direct
 * with n_rhs = 1 on member m's de-interleaved matrices and a one-member slod_lod_factor_create_zldl of the same
 * (alpha, beta); they do not depend on K, a leading dimension, the member's position, first_member or the run; one call
 * with n_steps = 2 equals two calls with n_steps = 1.  Padding entries >= n_members inside any ld are neither read nor
 * written.
 * SLOD_ERR_ARGUMENT, before any device work, with the call's name: everything the single calls refuse, with their
 * messages (n_members in the place of n_rhs); n_members < 1; ld_a_m, ld_m_m, ld_u, ld_v or ld_load below n_members;
 * first_member < 0 or first_member + n_members beyond the factor's members, "<call>: members outside the factor"; a real
 * factor, "<call>: takes a complex factor (slod_lod_factor_create_zldl)".  The single calls go on taking `member` of a
 * factor of several members; the real consumers go on refusing it.
 * Not built: several columns per member, three-stage schemes, CG or PCG as the stage solver, members spread over ranks,
 * the deal.II adapter.  The two steppers take a record armed by slod_lod_time_record_arm (below); its receivers hold
 * n_members members, read from member 0 whatever first_member. */
int slod_lod_irk_heat_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, int first_member, int scheme,
                                            const double *d_stiffness, size_t ld_a_m, const uint32_t *d_cols, double dt,
                                            int n_steps, int n_members, double *d_u, size_t ld_u,
                                            const double *d_load /* NULL = 0 */, size_t ld_load, size_t load_stage_stride);
int slod_lod_irk_wave_steps_ensemble_direct(slod_handle *h, slod_lod_factor *f_S, int first_member, int scheme,
                                            const double *d_stiffness, size_t ld_a_m, const double *d_mass, size_t ld_m_m,
                                            const uint32_t *d_cols, double dt, double damp_mass, double damp_stiff,
                                            int n_steps, int n_members, double *d_u, size_t ld_u, double *d_v, size_t ld_v,
                                            const double *d_load /* NULL = 0 */, size_t ld_load, size_t load_stage_stride,
                                            double *kinetic   /* HOST [(n_steps+1)*n_members], may be NULL */,
                                            double *potential /* HOST [(n_steps+1)*n_members], may be NULL */);

/* ---- receivers: the solution at a few points, as a product on the LOD space and as a trace of the time loops ----
 * Who runs a time loop wants the solution at a few points as a function of time: a seismogram, a sensor, a band on either
 * over an ensemble.  These calls evaluate (C u)(x) at chosen points without forming the fine field, and record it inside
 * the loops without cutting them into single steps.
 * A TERM is (global fine node < (NE+1)^2, component c < spacedim, weight w); a RECEIVER is a short list of terms, given
 * in CSR form on the host: receiver q owns the terms term_begin[q] .. term_begin[q+1]-1, term_begin[0] = 0.  One term of
 * weight 1 is a nodal value, four terms with bilinear weights the FE function at a point, two of opposite sign a
 * difference, a handful a small average.
 * ROWS.  The row of a term over the coarse unknowns is what slod_lod_reconstruct sums for that node and component, in its
 * order: the patches by centre cell cy, then cx, over the cells whose closed patch holds the node, then d = 0 .. s-1,
 * each giving the column p s + d and the value w phi_{p,d}(node, c), rounded once.  The rows of a receiver's terms are
 * concatenated in term order; equal columns are not merged; a patch whose rim holds the node stays in the row.  Storage is
 * CSR, row_begin[n_recv + 1], cols[nnz], values[nnz K] member-minor (entry e of member m at values[e K + m]) for the K
 * members of an ensemble slab laid out as for slod_lod_matrix_ensemble (d_basis, stride, member_stride; K = 1: one slab).
 * slod_lod_receiver_capacity: the bound (2 l + 2)^2 s on the entries of a term.  slod_lod_receiver_pattern: the columns
 * of the row of a term at `node` (they do not depend on the component), in row order; returns their count.  Both host only.
 * slod_lod_receivers_create reads the slab once (one gather kernel) and synchronises; the rows are not refreshed after
 * slod_update_coefficient: create the object again.  SLOD_ERR_ARGUMENT, before any device work, with the call's name: a
 * NULL handle, array or out; n_recv < 1; a receiver without terms; a term_begin that is not monotone; a node >= (NE+1)^2;
 * a component >= spacedim; a weight that is not finite; n_members < 1 or > 65535; a stride below the words of a patch; nnz
 * that does not fit 31 bits.  SLOD_ERR_DEVICE without a usable GPU.
 * THE PRODUCT y = O u on coarse multi-vectors: y of receiver q, column c at d_y[q ld_y + c].  slod_lod_observe_multi takes
 * an object of one member and applies its rows to every column; slod_lod_observe_ensemble reads for column m the values
 * of member first_member + m.  One thread per (receiver, column), one chain acc = fma(value_e, u[cols_e ld_u + c], acc)
 * from 0.0 over the row in order: a one-term receiver of weight 1 gives the 64-bit word slod_lod_reconstruct_multi /
 * slod_lod_reconstruct_ensemble writes at that node and component, and the bits of a column do not depend on the number
 * of columns, a leading dimension or the column's position.  Entries c >= n inside an ld are neither read nor written.
 * Asynchronous, no allocation.  SLOD_ERR_ARGUMENT: a NULL handle, receivers or array; n < 1; ld_u or ld_y below the
 * columns; the receivers of another handle; an object of several members given to slod_lod_observe_multi; members outside
 * the object.
 * THE RECORD.  slod_lod_time_record_arm leaves on the handle what the NEXT stepper call records:
 *   record j (0 .. n_steps / every), quantity w (u before v, of those asked for), receiver q, column c at
 *   d_trace[j record_stride + (w n_recv + q) ld_trace + c];
 * record j holds the state after j every steps, record 0 the entry state; with every = 3 and n_steps = 7 the state after
 * step 7 is not recorded.  The product is queued on the loop's stream after the entry state and after the advance of
 * every every-th step, u and v in one launch, inside the one queue-and-wait of the loops on a factor: nothing is allocated
 * and nothing is read back; when the stepper returns the trace is complete, on the device.  Words of d_trace outside these
 * positions are not written.  A loop without a record runs the code and has the bits it had before.
 * ONE-SHOT: the next call of slod_lod_theta_steps, _direct, _ensemble_direct, slod_lod_newmark_steps, _direct,
 * _ensemble_direct, slod_lod_irk_heat_steps_direct, slod_lod_irk_wave_steps_direct or their _ensemble_direct forms on this
 * handle takes the record off the handle as its first action and is the only call that sees it, whatever it returns.
 * Every other call leaves it alone (the slod_lod_newmark_accel calls too); rec = NULL disarms, and so does
 * slod_lod_receivers_destroy of the receivers it names.  The struct is copied; d_trace must live until the stepper has
 * returned.
 * A stepper with a record refuses with SLOD_ERR_ARGUMENT, before any device work, after its own checks and in this order,
 * "<call>: record: ...": SLOD_RECORD_V in a theta or heat loop; a `what` outside 1 .. 3; every < 1; a NULL d_trace; an
 * ld_trace below the columns of the call; a record_stride below n_quantities n_recv ld_trace; capacity < n_steps / every
 * + 1; the receivers of another handle; a member count that is not 1 for a single-problem stepper or not n_members for an
 * ensemble stepper (whose column m reads member m of the object).  slod_lod_time_record_arm itself refuses a NULL handle
 * and a NULL recv inside a non-NULL record.
 * Not built: time signals that scale a load inside the loop (sources) came later, see the next block; full-field snapshots every M steps; merging equal
 * columns of a row; receivers refreshed after slod_update_coefficient; records from the eigen and harmonic calls; members
 * spread over ranks; the deal.II adapter. */
typedef struct slod_lod_receivers slod_lod_receivers;
typedef struct
{
  int32_t  n_receivers, n_members;
  uint64_t nnz;   /* entries of the rows, per member */
  uint64_t bytes; /* device memory of the object */
} slod_lod_receivers_info;
int slod_lod_receiver_capacity(const slod_handle *h);
int slod_lod_receiver_pattern(const slod_handle *h, uint32_t node, uint32_t *cols /* HOST */, size_t capacity);
int slod_lod_receivers_create(slod_handle *h, int n_recv, const uint32_t *term_begin /* HOST [n_recv+1] */,
                              const uint32_t *term_node /* HOST */, const int32_t *term_comp /* HOST */,
                              const double *term_weight /* HOST */, const double *d_basis, size_t stride, size_t member_stride,
                              int n_members, slod_lod_receivers **out);
int slod_lod_receivers_get_info(const slod_lod_receivers *recv, slod_lod_receivers_info *info);
/* row_begin [n_recv + 1], cols [nnz] and the values [nnz] of one member to HOST arrays; synchronises the handle's stream */
int slod_lod_receivers_rows(const slod_lod_receivers *recv, int member, uint32_t *row_begin, uint32_t *cols, double *values);
void slod_lod_receivers_destroy(slod_lod_receivers *recv);
int slod_lod_observe_multi(slod_handle *h, const slod_lod_receivers *recv, const double *d_u, size_t ld_u, int n_rhs, double *d_y,
                            size_t ld_y, void *hip_stream);
int slod_lod_observe_ensemble(slod_handle *h, const slod_lod_receivers *recv, int first_member, int n_members, const double *d_u,
                               size_t ld_u, double *d_y, size_t ld_y, void *hip_stream);
enum slod_record_what { SLOD_RECORD_U = 1, SLOD_RECORD_V = 2 };
typedef struct
{
  const slod_lod_receivers *recv;
  int     what;          /* SLOD_RECORD_U = 1, SLOD_RECORD_V = 2, or both */
  int     every;         /* >= 1: record j holds the state after j * every steps, j = 0 is the entry state */
  double *d_trace;       /* DEVICE */
  size_t  ld_trace;      /* >= columns of the stepper call */
  size_t  record_stride; /* doubles between records, >= n_quantities * n_recv * ld_trace */
  int     capacity;      /* records d_trace can hold */
} slod_lod_time_record;
int slod_lod_time_record_arm(slod_handle *h, const slod_lod_time_record *rec /* NULL disarms */);

/* ---- sources: point forces with a time signal, as a product on the LOD space and as a load of the time loops ----
 * The other half of a seismogram.  A point force w e(node, c) has the coarse load C^T w e, which is the row of O = W C a
 * receiver at that term has: a set of sources is a receivers object applied transposed,  b = b_base + O^T g,  and a time
 * loop that knows the sources needs a wavelet per source and column in place of (n_steps + 1) n ld_load doubles of loads.
 * THE OBJECT.  slod_lod_sources_create takes a receivers object of the same handle; source q is receiver q, with its
 * terms, weights and members.  It reads the rows back, builds the transposed index on the host (the touched coarse rows,
 * ascending; per touched row the entries e with cols[e] = r in ascending e, so by source, term and row order; the source
 * q(e) of each entry; an int32 map coarse row -> slot, -1 if untouched, of num_patches s words) and copies the values
 * into that order, member-minor, with one gather kernel: the words are those of the receivers object.  The object owns
 * its copy; the receivers may be destroyed afterwards.  Synchronises.  Not refreshed after slod_update_coefficient: create
 * again.  SLOD_ERR_ARGUMENT: a NULL handle, recv or out; the receivers of another handle.
 * THE PRODUCT.  b of coarse row r, column c at d_b[r ld_b + c]; g of source q, column c at d_g[q ld_g + c]; d_base in the
 * layout of d_b, NULL = +0.0.  slod_lod_inject_multi takes an object of one member; slod_lod_inject_ensemble reads for
 * column m the values of member first_member + m.  One thread per (coarse row, column): an untouched row writes its base
 * word (any word, a NaN too, bit for bit); a touched row runs one chain acc = fma(value_e, g[q(e) ld_g + c], acc) from the
 * base word over its entries in the stored order.  A one-term source of weight 1 and signal 1 leaves in the touched rows
 * the words slod_lod_rhs_multi gives for the fine field e(node, c).  The words of a column depend on the object, the
 * member, that column of g and that column of the base alone.  d_b may be d_base.  Entries c >= n inside an ld are neither
 * read nor written.  Asynchronous, no allocation, no atomics.  SLOD_ERR_ARGUMENT: a NULL handle, sources or d_g / d_b;
 * n < 1; ld_g, ld_b or (with a base) ld_base below the columns; the sources of another handle; an object of several
 * members given to slod_lod_inject_multi; members outside the object.
 * THE ARMED SOURCE.  slod_lod_time_source_arm leaves on the handle what drives the NEXT stepper call: its load is d_load
 * (as before: NULL = zero, stride 0 = constant) PLUS O^T g(t), with the sample of g taken as the loads are: the theta
 * loops use sample k for b^k, k = 0 .. n_steps (n_samples >= n_steps + 1); Newmark uses sample k + 1 for step k (the same
 * bound); IRK uses sample 2 k + i for stage i of step k (n_samples >= 2 n_steps).  The armed loop carves two load vectors
 * of n x columns more (Newmark: one) out of its one workspace and queues one product per step on its stream ahead of the
 * right-hand side, which reads them in place of d_load; its words are those of an un-armed call on loads materialised by
 * slod_lod_inject_*.  Nothing else is allocated, nothing is read back, the loops on a factor stay one queue-and-wait.
 * An ensemble stepper reads member m of the object for column m, whatever first_member of its factor.  A loop without a
 * source runs the code and has the bits it had before.
 * ONE-SHOT, as the record: the next call of one of the ten steppers named there takes source and record off the handle as
 * its first action, whatever it returns; every other call leaves them (the slod_lod_newmark_accel calls too: their load at
 * t_0 is the caller's, slod_lod_inject_* forms it); s = NULL disarms, and so does slod_lod_sources_destroy of the sources
 * it names.  The struct is copied; d_signal must live until the stepper has returned.
 * A stepper with a source refuses with SLOD_ERR_ARGUMENT, before any device work, after its own checks and the record's
 * and in this order, "<call>: source: ...": a NULL d_signal; an ld_signal below the columns of the call; sample_stride /
 * n_sources < ld_signal; n_samples below the bound above; the sources of another handle; a member count that is not 1 for
 * a single-problem stepper or not n_members for an ensemble stepper.  slod_lod_time_source_arm itself refuses a NULL
 * handle and a NULL src inside a non-NULL struct.
 * Not built: sources in the slod_lod_newmark_accel, harmonic and eigen calls; a signal interpolated between samples;
 * sources refreshed after slod_update_coefficient; moving sources; members spread over ranks; the deal.II adapter. */
typedef struct slod_lod_sources slod_lod_sources;
typedef struct
{
  int32_t  n_sources, n_members;
  uint32_t n_rows_touched; /* coarse rows with an entry */
  uint64_t nnz;            /* entries, per member */
  uint64_t bytes;          /* device memory of the object */
} slod_lod_sources_info;
int slod_lod_sources_create(slod_handle *h, const slod_lod_receivers *recv, slod_lod_sources **out);
int slod_lod_sources_get_info(const slod_lod_sources *src, slod_lod_sources_info *info);
void slod_lod_sources_destroy(slod_lod_sources *src);
int slod_lod_inject_multi(slod_handle *h, const slod_lod_sources *src, const double *d_g, size_t ld_g, int n_rhs,
                          const double *d_base /* NULL = +0.0 */, size_t ld_base, double *d_b, size_t ld_b, void *hip_stream);
int slod_lod_inject_ensemble(slod_handle *h, const slod_lod_sources *src, int first_member, int n_members, const double *d_g,
                             size_t ld_g, const double *d_base /* NULL = +0.0 */, size_t ld_base, double *d_b, size_t ld_b,
                             void *hip_stream);
typedef struct
{
  const slod_lod_sources *src;
  const double *d_signal; /* DEVICE: sample j, source q, column c at d_signal[j sample_stride + q ld_signal + c] */
  size_t ld_signal;       /* >= columns of the stepper call */
  size_t sample_stride;   /* >= n_sources * ld_signal */
  int    n_samples;
} slod_lod_time_source;
int slod_lod_time_source_arm(slod_handle *h, const slod_lod_time_source *s /* NULL disarms */);

/* ---- sponge layers: a third damping matrix in the wave steppers and the frequency response ----
 * The calls above damp with Rayleigh's C = damp_mass M + damp_stiff A, the same everywhere, in a box with a homogeneous
 * Dirichlet rim: a wavelet returns from the rim.  A sponge is a coefficient sigma(x) >= 0 that is zero in the region of
 * interest and grows towards the rim.  These calls take the model
 *   M u'' + (damp_mass M + damp_stiff A + D) u' + A u = b(t)
 * with D a full set of block rows on the d_cols of A and M, typically slod_lod_mass_matrix(.., d_rho = sigma, ..), that is
 * D_LOD = C^T M_sigma C, bit-symmetric like M_LOD.  Any symmetric positive semi-definite matrix in that layout is allowed;
 * it may have zero rows (be rank deficient).  Semi-definiteness is the caller's business, as the positivity of a shift is
 * elsewhere: nothing checks it, and a D with a negative direction feeds energy.
 * In every call d_damping == NULL means D = 0: the call then runs the launches and returns the 64-bit words of the call
 * it extends, whose arguments it takes with d_damping after d_mass.  Each refuses what the extended call refuses, with
 * its own name in the text, SLOD_ERR_ARGUMENT before any device work.  A record and a source armed on the handle serve
 * the damped steppers as they serve their namesakes.
 * NEWMARK.  slod_lod_newmark_accel_damped, slod_lod_newmark_steps_damped (CG) and their _direct forms.
 *   acceleration   M a = b^0 - A (u + damp_stiff v) - damp_mass M v - D v
 *   step matrix    S = (1 + gamma dt damp_mass) M + (beta dt^2 + gamma dt damp_stiff) A + (gamma dt) D
 *   step rhs       g = ((b - A w) - damp_mass (M v~)) - (D v~), each product and difference rounded on its own; M v~ and D v~
 *                  are two fma chains in the slot order of slod_lod_apply_multi on one read of the row's column indices
 *                  and of v~; with damp_mass = 0 the D chain runs alone.
 * The CG forms build S in the call's workspace as two slod_lod_matrix_combine roundings: (c_M M + c_A A), then that + c_D D
 * (1.0 times the first sum is exact, so S = fl(fl(fl(c_M M) + fl(c_A A)) + fl(c_D D))).  The _direct forms take the
 * caller's factor of that S, Cholesky or LDL^T, and the factor of M for the acceleration.  Predictor, corrector, energies
 * (1/2 v^T M v, 1/2 u^T A u), n_steps = 2 == 2 x 1, column independence stay as they are.  For beta = 1/4, gamma = 1/2 and no
 * load the energy obeys  E_{k+1} - E_k = -dt vbar^T C vbar,  vbar = (v_k + v_{k+1}) / 2.
 * COMPLEX FACTOR.  slod_lod_factor_create_zldl3 factors S_k = alpha_k A + beta_k B + gamma_k C, gamma HOST [n_members][2]
 * like alpha and beta.  Band word: re = ((alpha_re a) + (beta_re b)) + (gamma_re c), the imaginary plane alike, every product
 * and sum rounded on its own.  Everything else is slod_lod_factor_create_zldl: its error texts with the new name, the
 * independence of a member's words from n_members and its position, slod_lod_factor_solve_complex, get_info and inertia,
 * and every real consumer refuses the object.  SLOD_ERR_ARGUMENT: a NULL handle, array (d_c too), alpha, beta, gamma or
 * out; n_members < 1 or > 65535; a coefficient (of gamma too) that is NaN or infinite.
 * IRK.  slod_lod_irk_damping_coefficient (host only) returns gamma = z = dt lambda of the scheme, formed in long double and
 * rounded once per part; it refuses a NULL gamma, an unknown scheme and dt <= 0, NaN or infinite, as
 * slod_lod_irk_coefficients does.  slod_lod_irk_wave_steps_damped_direct runs on a member of
 *   S = (1 + z damp_mass) M + (z damp_stiff + z^2) A + z D,
 * slod_lod_factor_create_zldl3 with the pair of slod_lod_irk_coefficients(scheme, 2, ..) and gamma = z.  Re S stays
 * symmetric positive definite because Re z > 0, so the factor exists without pivoting.
 *   r = tau_1 b_1 + tau_2 b_2 - sigma [A (u + (z + damp_stiff) v) + damp_mass M v + D v],   the update is unchanged;
 * D v is a fourth fma chain next to A u, A v and M v on the same loads of v.
 * FREQUENCY RESPONSE.  slod_lod_harmonic_response_damped, with a trailing quantities (HOST [n_freq * n_rhs][5], may be NULL):
 *   S(omega) = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M + i omega D,   gamma_k = (0, omega_k).
 * It works in chunks of 64 frequencies, waited for once each.  The true residual is formed from the three matrices: six
 * row products in one launch.  quantities[(k n_rhs + c)] = (u^H M u, u^H A u, u^H D u, Re u^H b, Im u^H b) with the roundings
 * and the fixed summation order of the ensemble call's quantities (u^H D u is +0.0 without D); a zero load column gives
 * five zeros.  They balance:  omega (damp_mass u^H M u + damp_stiff u^H A u + u^H D u) = Im u^H b,  the imaginary part of
 * u^H S u = u^H b; the real part is u^H A u - omega^2 u^H M u = Re u^H b.
 * With damp_mass = damp_stiff = 0 and a D that is only semi-definite the imaginary part of S is not definite: the
 * existence of the factor is then the caller's risk and the growth is reported, as for omega = 0 in
 * slod_lod_harmonic_response.
 * Not built: ensemble forms of the four damped calls and of slod_lod_factor_create_zldl3; theta-scheme or heat calls
 * (damping is second order only); the eigen calls (a quadratic eigenproblem); perfectly matched layers (they change A);
 * a refresh of D after slod_update_coefficient (rebuild it with slod_lod_mass_matrix); the deal.II adapter. */
int slod_lod_newmark_accel_damped(slod_handle *h, const double *d_stiffness, const double *d_mass,
                                  const double *d_damping /* NULL: D = 0 */, const uint32_t *d_cols, double damp_mass,
                                  double damp_stiff, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                                  const double *d_load, size_t ld_load, double *d_a, size_t ld_a, double rel_tol, int max_iterations,
                                  int *iterations, double *rel_residual);
int slod_lod_newmark_steps_damped(slod_handle *h, const double *d_stiffness, const double *d_mass,
                                  const double *d_damping /* NULL: D = 0 */, const uint32_t *d_cols, double dt, double beta,
                                  double gamma, double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u, size_t ld_u,
                                  double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load, size_t ld_load,
                                  size_t load_step_stride, double rel_tol, int max_iterations, int *iterations, double *rel_residual,
                                  double *kinetic, double *potential);
int slod_lod_newmark_accel_damped_direct(slod_handle *h, slod_lod_factor *f_M, const double *d_stiffness, const double *d_mass,
                                         const double *d_damping /* NULL: D = 0 */, const uint32_t *d_cols, double damp_mass,
                                         double damp_stiff, int n_rhs, const double *d_u, size_t ld_u, const double *d_v, size_t ld_v,
                                         const double *d_load, size_t ld_load, double *d_a, size_t ld_a);
int slod_lod_newmark_steps_damped_direct(slod_handle *h, slod_lod_factor *f_S, const double *d_stiffness, const double *d_mass,
                                         const double *d_damping /* NULL: D = 0 */, const uint32_t *d_cols, double dt, double beta,
                                         double gamma, double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u,
                                         size_t ld_u, double *d_v, size_t ld_v, double *d_a, size_t ld_a, const double *d_load,
                                         size_t ld_load, size_t load_step_stride, double *kinetic, double *potential);
int slod_lod_factor_create_zldl3(slod_handle *h, const double *d_a, const double *d_b, const double *d_c, const uint32_t *d_cols,
                                 const double *alpha /* HOST [n_members][2] */, const double *beta, const double *gamma,
                                 int n_members, int32_t *bad_pivot /* HOST [n_members], may be NULL */, slod_lod_factor **out);
int slod_lod_irk_damping_coefficient(int scheme, double dt, double gamma[2]);
int slod_lod_irk_wave_steps_damped_direct(slod_handle *h, slod_lod_factor *f_S, int member, int scheme, const double *d_stiffness,
                                          const double *d_mass, const double *d_damping /* NULL: D = 0 */, const uint32_t *d_cols,
                                          double dt, double damp_mass, double damp_stiff, int n_steps, int n_rhs, double *d_u,
                                          size_t ld_u, double *d_v, size_t ld_v, const double *d_load, size_t ld_load,
                                          size_t load_stage_stride, double *kinetic, double *potential);
int slod_lod_harmonic_response_damped(slod_handle *h, const double *d_stiffness, const double *d_mass,
                                      const double *d_damping /* NULL: D = 0 */, const uint32_t *d_cols, double damp_mass,
                                      double damp_stiff, const double *omega /* HOST [n_freq] */, int n_freq, const double *d_load_re,
                                      const double *d_load_im, size_t ld_load, int n_rhs, double *d_u_re, double *d_u_im, size_t ld_u,
                                      double *rel_residual, double *growth, double *quantities /* HOST [n_freq*n_rhs][5], may be NULL */);

/* ---- refresh after a local coefficient change ----------------------------------------------
 * Every entry point above takes the coefficient as fixed for the life of a basis (the reference does too: one
 * compute_basis_function_candidates per run, LOD.cc:1425-1433).  When it changes in a small part of the domain -- a
 * moving inclusion, a growing damage zone, a local perturbation in a parameter study -- only the patches whose extent
 * holds a changed fine element have another basis, and only the entries of A_LOD and M_LOD with such a patch as row or
 * column have another value.  These calls find those patches, rebuild them in place and recompute those entries in
 * place, each with the bits a full rebuild gives (see slod_plan_create_dirty for the one exception).
 * A DIRTY ARRAY is a caller-owned DEVICE array of num_patches uint32_t, one word per patch of ONE problem; a non-zero
 * word means the patch is dirty.  The caller zeroes it (hipMemsetAsync) and may set words by hand.
 * Not covered: a change of rho (rebuild M_LOD), C^T f of the dirty rows (slod_lod_rhs with the list of
 * slod_dirty_patches, or the whole load: either is one read of the slab), handles with constant_coefficients = 1. */
/* slod_set_coefficient (same arguments, layouts, host or device data; runs on the handle's stream and synchronises)
 * that also ORs 1 into d_dirty[p] for every patch p whose extent, the fine elements [x0 n, (x0 + mx) n) x
 * [y0 n, (y0 + my) n) with n = n_subdivisions, holds a changed element.  An element is changed when at least one of
 * its four stored values differs from the stored field AS A 64-BIT WORD: no tolerance, 1.0 -> nextafter(1.0) is a
 * change, the same bits are none.  Words of clean patches are left as they are, so flags accumulate over calls: the
 * two Lame fields take two calls on one array.
 * Checked in this order, all before any device work: SLOD_ERR_ARGUMENT: what slod_set_coefficient refuses, or a NULL
 * d_dirty; SLOD_ERR_UNSUPPORTED: constant_coefficients = 1 (under quirk Q1 every full patch reads the first full
 * patch's tile, so its basis does not depend on its own elements); SLOD_ERR_STATE: (problem, field) has never been
 * set; SLOD_ERR_DEVICE without a usable GPU. */
int slod_update_coefficient(slod_handle *h, uint32_t problem, int field, const double *data, int layout,
                            size_t count, int on_device, uint32_t *d_dirty);
/* Number of dirty patches; `patches` (HOST, may be NULL) receives their ids in ascending order.  SLOD_ERR_ARGUMENT
 * when capacity is below the count; patches = NULL, capacity = 0 only counts.  Synchronises the handle's stream and
 * reads the array back with a blocking copy. */
int slod_dirty_patches(slod_handle *h, const uint32_t *d_dirty, uint32_t *patches /* HOST, may be NULL */, size_t capacity);
/* Returns the number n >= 0 of dirty patches and sets *out to the plan slod_plan_create gives for the gids
 * problem * num_patches + p of the dirty patches p, ascending, with offsets[k] = p * slod_plan_stride(): executed on the
 * uniform-stride slab of the problem it overwrites the dirty patches in place and writes nothing else (not the gap up
 * to the stride either).  n = 0: the empty plan, whose execute does nothing.  Synchronises like slod_dirty_patches.
 * Contract on the bits: they are those of that slod_plan_create call.  The patch-solve kernel of a plan is chosen from
 * the plan's maxima over its patches (line length, coarse dofs, ...), so a dirty list without a full patch may run
 * another kernel instantiation than the plan over all patches and then differs from a full rebuild in the last bits;
 * a list that holds a full patch has the maxima of the full plan. */
int slod_plan_create_dirty(slod_handle *h, uint32_t problem, const uint32_t *d_dirty, slod_plan **out);
/* In place on a full set of block rows (rows 0 .. num_patches-1 in the layout of slod_lod_matrix, or one member of an
 * ensemble matrix: d_values + k, ld_m, with that member's slabs): recomputes every used entry (p, j) with
 * d_dirty[p] != 0 or d_dirty[q] != 0, q the column of slot j.  Each recomputed entry has the bits of slod_lod_matrix /
 * slod_lod_matrix_ensemble on the current slabs; no other word of d_values is written.  d_cols is not needed: it
 * depends on the grid only.  One block per row; a clean row far from any dirty patch costs its row-capacity flag loads.
 * Uploads nothing: ASYNCHRONOUS on hip_stream.  SLOD_ERR_ARGUMENT: NULL handle or array, ld_m < 1. */
int slod_lod_matrix_update(slod_handle *h, const uint32_t *d_dirty, const double *d_basis, const double *d_premult,
                           size_t stride, double *d_values, size_t ld_m, void *hip_stream);
/* The same for M_LOD: the used entries with a dirty p or q get the bits of slod_lod_mass_matrix with the same d_rho
 * (NULL = 1).  (p, q) and (q, p) are always recomputed together, so the matrix stays symmetric bit for bit.
 * Asynchronous on hip_stream.  SLOD_ERR_ARGUMENT: NULL handle, d_dirty, d_basis or d_values. */
int slod_lod_mass_matrix_update(slod_handle *h, const uint32_t *d_dirty, const double *d_basis, size_t stride,
                                const double *d_rho, double *d_values, void *hip_stream);

/* ---- fine FEM reference problem (assemble_and_solve_fem_problem, LOD.cc:1004-1094) ----
 * What the reference compares the LOD solution with (compare_lod_with_fem, LOD.cc:1240-1378).
 * fem_rhs of assemble_stiffness (Diffusion.h:149-193) on the global fine grid, [(NE+1)^2][s],
 * zero on the Dirichlet nodes (all sides, LOD.cc:1021): d_f_qp = right-hand side function at the
 * quadrature points, DEVICE, [s][NE][NE][4] with the layout of slod_set_coefficient, or NULL for
 * f = (1,..,1) (the example's "fem rhs l2 norm = 0.109375", tests/Poisson_LOD_Example.output).
 * Asynchronous on hip_stream. */
int slod_fem_rhs(slod_handle *h, const double *d_f_qp, double *d_fine_rhs, void *hip_stream);
/* Fine FEM solution for the coefficient of `problem` (the reference: CG + AMG, LOD.cc:1070-1075;
 * here a matrix-free Jacobi-preconditioned CG on the 9-point stencil planes, all on the device).
 * Returns the iteration count (>= 0) or a negative slod_status; *rel_residual (HOST, may be
 * NULL) receives ||r|| / ||rhs||.  d_fine_u: DEVICE, [(NE+1)^2][s], zero on the boundary.
 * Synchronises. */
int slod_fem_solve(slod_handle *h, uint32_t problem, const double *d_fine_rhs, double *d_fine_u, double rel_tol,
                   int max_iterations, double *rel_residual);

/* ---- coarse FEM(H) reference problem (the coarse part of assemble_and_solve_fem_problem,
 * LOD.cc:1103-1237) ----
 * Q1 on the COARSE mesh (N x N cells, H = 1/N; FE_Q_iso_Q1(1) with QIterated(QGauss(2), 1), the reference's
 * coarse_fem_subdivisions = 1), the coefficient sampled at the 2 x 2 Gauss points of every coarse cell
 * (assemble_stiffness_coarse, Diffusion.h:210-305, Elasticity.h:304ff): the baseline with the number of
 * unknowns of the LOD system and no correctors.  Coarse nodal vectors are [(N+1)^2][s], lexicographic,
 * component-minor; coarse quadrature data is [N][N][4], q = q0 + 2 q1 at ((Cx + g[q0]) H, (Cy + g[q1]) H):
 * the layouts of the fine problem with NE -> N.
 * Common to the four calls: SLOD_ERR_ARGUMENT for a NULL handle or array, a problem or a field (>= spacedim)
 * out of range, before any device work; SLOD_ERR_DEVICE without a usable GPU; SLOD_ERR_STATE when the
 * coefficient the call reads has not been set.
 *
 * The coefficient of (problem, field) at the coarse Gauss points, DEVICE out [N][N][4]; exposed for parity
 * tests and callers that assemble their own coarse operator.  The stored fine field [NE][NE][4] is read as
 * piecewise constant on the quadrants of the fine elements, which is what problem_parameter::value
 * (Diffusion.h:40-53) gives whenever 2^r <= 2 NE: the point (Cx + g[q0]) H lies in fine element
 * ex = Cx n + floor(n g[q0]) at local coordinate xi = n g[q0] - floor(n g[q0]) and reads its slot
 * q0' = (xi >= 1/2); the same in y.  With n_subdivisions = 1 the output is the fine field.  Asynchronous on
 * hip_stream. */
int slod_coarse_coefficient(slod_handle *h, uint32_t problem, int field, double *d_out, void *hip_stream);
/* Coarse load vector (fem_coarse_rhs of assemble_stiffness_coarse, Diffusion.h:210-305) [(N+1)^2][s], zero on
 * the Dirichlet nodes; d_f_cqp = f at the coarse Gauss points, DEVICE [s][N][N][4], or NULL for f = (1,..,1).
 * Asynchronous on hip_stream. */
int slod_coarse_fem_rhs(slod_handle *h, const double *d_f_cqp, double *d_coarse_rhs, void *hip_stream);
/* FEM(H) solution [(N+1)^2][s] for the coefficient of `problem`, zero on the boundary (the reference:
 * SolverDirect, LOD.cc:1191-1197; here the solver of slod_fem_solve on the coarse grid: run it to a tight
 * tolerance).  Returns the iteration count (>= 0) or a negative slod_status, *rel_residual as slod_fem_solve.
 * Synchronises. */
int slod_coarse_fem_solve(slod_handle *h, uint32_t problem, const double *d_coarse_rhs, double *d_coarse_u,
                          double rel_tol, int max_iterations, double *rel_residual);
/* fem_coarse_solution_interpolated (FETools::interpolate, LOD.cc:1201-1204): bilinear interpolation of a
 * coarse nodal field onto the fine grid, DEVICE [(NE+1)^2][s]; fine nodes on coarse nodes copy the value bit
 * for bit.  Asynchronous on hip_stream.
 * The error tables of the coarse problem need no norm kernel of their own: every fine element lies inside
 * one coarse cell, so the fine-grid quadrature of slod_compute_error_norms is exact for the interpolated
 * field.  "FEM(H) vs reference FEM(h)" (LOD.cc:1206-1217,1458-1459) is slod_compute_error_norms(u = fem_h,
 * v = interpolated), "FEM(H) vs exact solution" (LOD.cc:1450-1451) the same call with u = interpolated and
 * the exact arrays. */
int slod_coarse_interpolate(slod_handle *h, const double *d_coarse, double *d_fine, void *hip_stream);

/* ---- error norms on the global fine grid (compare_lod_with_fem, LOD.cc:1240-1260:
 * error_LOD_FEMh.difference and error_LOD_exact.error_from_exact; error_FEMh_exact, LOD.cc:1080-1088;
 * the tables printed at the end of run(), LOD.cc:1425-1466) ----
 * e = u - v - w, with u, v DEVICE nodal Q1 fields [(NE+1)^2][s] (the layout of slod_fem_solve and
 * slod_lod_reconstruct; NULL = 0) and w an optional exact function given at the quadrature points:
 * d_exact_qp [s][NE][NE][4] values, d_exact_grad_qp [s][2][NE][NE][4] gradients (d = 0: x, 1: y), both
 * DEVICE, 16-byte aligned, and given together or both NULL.  The points are those of slod_set_coefficient
 * layout 1 and of slod_fem_rhs's d_f_qp: q = q0 + 2 q1 at ((ex + g[q0]) h, (ey + g[q1]) h),
 * g = 1/2 -+ 1/(2 sqrt 3), h = 1/NE: the 2 x 2 Gauss rule of the fine stiffness (QIterated(QGauss(2), n),
 * LOD.cc:91-92) on every fine element, which is what every integral below uses.
 *   l2[c]      = (int e_c^2)^{1/2}           h1_semi[c] = (int |grad e_c|^2)^{1/2}
 *   linf[c]    = max over the quadrature points of |e_c|       (entries c >= spacedim are 0)
 *   energy     = a(e,e)^{1/2} with the coefficient of `problem`: int alpha |grad e|^2 (spacedim 1),
 *                int 2 mu eps(e):eps(e) + lambda (div e)^2 (spacedim 2, Elasticity.h:245-254).
 * For FE fields (w NULL) energy^2 equals e^T A_h e of the unconstrained fine stiffness up to rounding.
 * deal.II's H1_norm is the full norm (l2^2 + h1_semi^2)^{1/2}; ParsedConvergenceTable sums components
 * of the same name in squares.  deal.II's error_from_exact integrates with a quadrature of its own, so
 * errors against an exact solution are comparable to the reference's but not bit-equal.
 * The reduction has a fixed order (no atomics): the same inputs give bitwise the same result.
 * SLOD_ERR_ARGUMENT: NULL h or out, problem out of range, only one of the exact arrays, misaligned
 * exact arrays; SLOD_ERR_DEVICE: no usable GPU; SLOD_ERR_STATE: coefficient of `problem` not set.
 * The handle owns the reduction workspace (allocated on first use).  hip_stream NULL = the handle's
 * stream; the call SYNCHRONISES hip_stream. */
typedef struct
{
  double l2[2];      /* ||e_c||_L2, c < spacedim (unused entries 0)            */
  double h1_semi[2]; /* |e_c|_H1                                              */
  double linf[2];    /* max over quadrature points |e_c|                      */
  double energy;     /* a(e,e)^{1/2} with the coefficient of `problem`         */
  double reserved[3];
} slod_error_norms;
int slod_compute_error_norms(slod_handle *h, uint32_t problem, const double *d_u, const double *d_v,
                             const double *d_exact_qp, const double *d_exact_grad_qp, slod_error_norms *out,
                             void *hip_stream);

/* ---- inputs of the path produced on the device --------------------------------------
 * create_patches + create_mesh_for_patch + fill_dofs_indices_vector (LOD.cc:122-244,
 * 770-858; LODtools.h:334-375) evaluated by a kernel, one thread per patch; out is a HOST
 * array of n entries, equal to slod_patch_layout() entry by entry (tests check both against
 * the reference golden tests/create_patch_01.output). */
int slod_device_patch_layout(slod_handle *h, const uint32_t *patch_ids, size_t n, slod_patch_info *out);
/* The reference's coefficient object problem_parameter(min, max, r) (Diffusion.h:7-54): a
 * piecewise constant on a 2^r x 2^r grid, value(p) = vals[floor(x / eta) + 2^r floor(y / eta)],
 * eta = 2^-r (:47-51), sampled ON THE DEVICE at the points of quadrature_fine of every fine
 * element (what Alpha.value_list does at Diffusion.h:154).  d_vals: DEVICE, 4^r values in
 * the reference's fill order (:30-36). */
int slod_sample_coefficient(slod_handle *h, uint32_t problem, int field, const double *d_vals, int r);

/* ---- multi-GPU exchange (north_star: RCCL all-gather over xGMI of the basis vectors) ----
 * The reference never communicates basis vectors (its MPI path is unfinished, LOD.cc:225-229,
 * 895-897); the split it prescribes is contiguous blocks of patch ids per rank (LOD.cc:116-118,
 * slod_partition).  One process per GPU; the C/C++ host exchanges the 128-byte id out of band
 * (MPI_Bcast in dealii-slod) and then needs nothing but this library: RCCL is resolved at run
 * time (no link-time dependency; a process that already runs RCCL re-uses that copy). */
typedef struct
{
  char internal[128]; /* ncclUniqueId */
} slod_comm_id;
typedef struct slod_comm slod_comm;
const char *slod_comm_last_error(const slod_comm *c); /* c may be NULL: last failed create */
int         slod_comm_unique_id(slod_comm_id *id);    /* on rank 0; ship it to the other ranks */
int         slod_comm_create(const slod_comm_id *id, int n_ranks, int rank, int device, slod_comm **out);
void        slod_comm_destroy(slod_comm *c);
/* plain ncclAllGather of `count` doubles per rank on hip_stream (uniform-stride slabs) */
int slod_comm_allgather(slod_comm *c, const double *d_send, double *d_recv, size_t count, void *hip_stream);
/* Patch range [first, first + count) of piece `piece` out of n_pieces of a rank's padded slab of
 * patches_per_rank patches (host-only index calculus of slod_plan_execute_allgather). */
int slod_gather_piece(uint64_t patches_per_rank, uint32_t n_pieces, uint32_t piece, uint64_t *first,
                      uint64_t *count);
/* Basis construction of this rank's patches and their exchange, overlapped: the plan (uniform
 * stride, at most patches_per_rank patches) is executed in n_pieces pieces on compute_stream
 * into this rank's slab  d_*_all + rank * patches_per_rank * stride;  as soon as a piece is
 * done, comm_stream exchanges that piece of EVERY rank (grouped in-place broadcasts, one per
 * root) while the next piece is computed.  On return (asynchronous) compute_stream is ordered
 * after the exchange.  Every rank must call it with the same patches_per_rank and n_pieces.
 * Error path: a rank that fails before the grouped broadcasts are issued returns non-zero WITHOUT
 * entering the collective; its peers then wait inside RCCL.  Treat a non-zero return on any rank as
 * fatal for the communicator (destroy it, or abort the job): there is no recovery inside the call. */
int slod_plan_execute_allgather(slod_plan *p, slod_comm *c, double *d_basis_all, double *d_premult_all,
                                size_t patches_per_rank, int n_pieces, void *compute_stream,
                                void *comm_stream);

/* ---- pieces exposed for parity tests ----------------------------------------------- */
/* unconstrained patch stiffness (replaces assemble_stiffness with empty constraints,
 * LOD.cc:440-444 -> Diffusion.h:111-207 / Elasticity.h:163-299) as a 9-point block stencil:
 * stencil[node][dir][a][b], dir = (dy+1)*3+(dx+1).  HOST buffer of n_nodes*9*s*s doubles. */
int slod_assemble_stiffness_for_patch(slod_handle *h, uint32_t gid, double *stencil);
/* Ainv_PT of Gauss_elimination (LOD.cc:546): HOST buffer [n_fine][n_coarse] row-major. */
int slod_patch_solution(slod_handle *h, uint32_t gid, double *X);

#ifdef __cplusplus
}
#endif
#endif /* SLOD_H */
