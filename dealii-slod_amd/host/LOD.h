// Host-side C++ mirror of the reference's class interface for the basis-construction path
// (reference include/LOD.h:68-262, source/LOD.cc), without deal.II: same class and member
// names, same argument meaning, same error behaviour (exceptions, as AssertThrow does in
// LODtools.h:416-438).  compute_basis_function_candidates() is the drop-in body: it calls
// the HIP library through the C-ABI of include/slod.h.  The steps of the reference run() after the
// basis build (assemble_global_matrix, assemble_and_solve_fem_problem, solve, compare_lod_with_fem:
// LOD.cc:860-1260) are public methods that chain the device entry points; run() stops after the
// basis build as before.  The coarse FEM(H) comparison (LOD.cc:1103-1237) is the public method
// assemble_and_solve_coarse_fem_problem().  VTU output is not mirrored.
#ifndef slod_host_lod_h
#define slod_host_lod_h

#include "../../include/slod.h"

#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace slod
{
  template <int dim>
  struct Point
  {
    std::array<double, dim> x{};
    double operator()(const unsigned int i) const { return x[i]; }
    double &operator()(const unsigned int i) { return x[i]; }
  };

  // dealii::Function<dim> as far as the path uses it (Diffusion.h:40-53,154)
  template <int dim>
  class Function
  {
  public:
    virtual ~Function() = default;
    virtual double value(const Point<dim> &p, const unsigned int component = 0) const = 0;
    void value_list(const std::vector<Point<dim>> &points, std::vector<double> &values,
                    const unsigned int component = 0) const
    {
      values.resize(points.size());
      for (std::size_t i = 0; i < points.size(); ++i)
        values[i] = value(points[i], component);
    }
  };

  // What create_mesh_for_patch() leaves in Patch::sub_tria (LOD.cc:770-858), reduced to what
  // the path reads: the cell box and the boundary id of each side (0 = domain boundary,
  // 99 = SPECIAL_NUMBER, LOD.cc:7).
  struct PatchMesh
  {
    unsigned int x0 = 0, y0 = 0, mx = 0, my = 0; // coarse cells
    unsigned int nx = 0, ny = 0;                 // fine elements
    std::array<unsigned int, 4> boundary_id{{99, 99, 99, 99}}; // left, right, bottom, top
    unsigned int n_active_cells() const { return mx * my; }
  };

  // reference include/LOD.h:68-82
  template <int dim>
  class Patch
  {
  public:
    std::vector<unsigned int>        cells; // vector_cell_index, centre first (LOD.cc:151-178)
    PatchMesh                        sub_tria;
    std::vector<std::vector<double>> basis_function;               // [spacedim][n_fine], deal.II dof order
    std::vector<std::vector<double>> basis_function_premultiplied; // [spacedim][n_fine]
    std::vector<unsigned int>        dealii_to_lexicographic;      // dof renumbering of the patch
    unsigned int                     contained_patches = 0;
  };

  // reference include/LOD.h:85-157 (the members the path reads) + the two quirk switches
  template <int dim, int spacedim>
  class LODParameters
  {
  public:
    unsigned int oversampling          = 1;
    unsigned int n_subdivisions        = 2;
    unsigned int n_global_refinements  = 2;
    bool         LOD_stabilization     = false;
    bool         constant_coefficients = true; // quirk Q1 when the coefficient is not constant
    bool         projection_quirk      = false; // quirk Q2 (LODtools.h:43-67), spacedim 2 only
    int          device                = 0;
    // coefficient realisations the handle holds (slod_config.n_problems); member 0 is the problem of run(), the others
    // are used by solve_ensemble() only
    unsigned int n_members             = 1;
  };

  template <int dim, int spacedim>
  class LOD
  {
  public:
    explicit LOD(const LODParameters<dim, spacedim> &par);
    virtual ~LOD();
    LOD(const LOD &) = delete;

    // make_grid, make_fe, initialize_patches, create_random_problem_coefficients,
    // compute_basis_function_candidates (LOD.cc:1425-1433); stops there.
    virtual void run();

    const std::vector<Patch<dim>> &get_patches() const { return patches; }
    // wall time of the last compute_basis_function_candidates() [s]
    double basis_build_seconds() const { return last_build_seconds; }

    // The rest of the reference run() (LOD.cc:1430-1433), after run(); one process owning every patch.
    // A_LOD = C^T (A C) from the basis, uploaded once as a uniform-stride slab (LOD.cc:860-973)
    void assemble_global_matrix();
    // fine FEM solution u_h with f = 1 (LOD.cc:1004-1094)
    void assemble_and_solve_fem_problem();
    // A_LOD u_H = C^T f_h (LOD.cc:976-1002)
    void solve();
    // u_LOD = C u_H and the norms of u_h - u_LOD (error_LOD_FEMh.difference, LOD.cc:1240-1260)
    void compare_lod_with_fem();
    // A factor that outlives a coefficient change.  factor_for_reuse(): the banded Cholesky factor of sym(A_LOD) as it
    // stands (slod_lod_matrix_symmetrize, slod_lod_factor_create), kept by this object.  solve_precond(): the system of
    // solve() on sym(A_LOD) as it stands then -- after refresh_after_coefficient_change() the refreshed matrix -- by CG
    // preconditioned by the kept, by then stale, factor (slod_lod_solve_multi_precond, n_rhs = 1), and by Jacobi-CG
    // (slod_lod_solve_multi) on the same system for the count next to it.  solve() itself stays on Jacobi-CG, and the K
    // loads of solve_multi() have no preconditioned form here: that is slod_lod_solve_multi_precond with n_rhs = K.
    void                factor_for_reuse();
    void                solve_precond();
    int                 precond_iterations() const { return lod_pcg_iterations; }
    int                 precond_jacobi_iterations() const { return lod_pcg_jacobi_iterations; }
    std::vector<double> precond_solution() const;
    // solve() for K load functions at once, after assemble_global_matrix() (the reference has a single load):
    // the fine load vectors of loads[k] sampled at the quadrature points, then C^T F, A_LOD U = C^T F and
    // U_fine = C U through slod_lod_rhs_multi / slod_lod_solve_multi / slod_lod_reconstruct_multi.
    void solve_multi(const std::vector<const Function<dim> *> &loads);
    const std::vector<int>    &multi_iterations() const { return lod_multi_iterations; }
    const std::vector<double> &multi_rel_residuals() const { return lod_multi_residuals; }
    // per load: the fine FEM solution of that load and the norms of u_h - u_LOD (compare_lod_with_fem per column)
    void compare_multi_with_fem();
    const std::vector<slod_error_norms> &error_multi_LOD_FEMh() const { return lod_multi_fem_error; }
    // M_LOD = C^T M C (consistent Q1 mass, density 1) in the pattern of A_LOD, after assemble_global_matrix() (the
    // reference has no counterpart: it has no time-dependent problem)
    void assemble_mass_matrix();
    // A sponge layer: D_LOD = C^T M_sigma C (slod_lod_mass_matrix with the density sigma per fine element, [NE * NE], ex
    // fastest, sigma >= 0) in the pattern of A_LOD, after assemble_global_matrix().  Once it is set, solve_wave,
    // solve_wave_irk and solve_harmonic add D u' to the model (the slod_lod_*_damped calls and slod_lod_factor_create_zldl3)
    // and solve_harmonic's power includes u^H D u.  damping_zero_rows(): the coarse rows of D that are zero.
    void         assemble_damping_matrix(const std::vector<double> &sigma);
    unsigned int damping_zero_rows() const { return lod_damping_zero_rows; }
    // n_steps of the theta scheme for M u' + A u = C^T f_h from u = 0 with the load of solve(), constant in time,
    // through slod_lod_theta_steps; after assemble_mass_matrix() and assemble_and_solve_fem_problem()
    // direct: the steps run on the banded Cholesky factor of S = M + theta dt A_LOD (lower triangle; factor_lod_matrix,
    // slod_lod_theta_steps_direct) and there are no iteration counts or residuals
    void solve_heat(const unsigned int n_steps, const double dt, const double theta, const bool direct = false);
    // The banded Cholesky factor of a symmetric positive definite matrix on the pattern of A_LOD (device values in the
    // layout of slod_lod_matrix): slod_lod_factor_create; the object owns the factor and frees it with itself.
    // last_factor_info() describes the factor made last.
    // ldl: the banded LDL^T factor of a symmetric, possibly indefinite matrix instead (slod_lod_factor_create_ldl, no
    // pivoting); last_factor_inertia() then holds the signs of D, ||S||_inf and || |L||D||L^T| ||_inf of member 0.
    slod_lod_factor            *factor_lod_matrix(const double *d_values, const bool ldl = false);
    // the complex LDL^T of alpha sym(A_LOD) + beta M_LOD (d_lod_sym must hold the symmetrised stiffness), owned like the others
    slod_lod_factor            *factor_lod_irk(const int scheme, const int order, const double dt);
    const slod_lod_factor_info &last_factor_info() const { return lod_factor_info; }
    const slod_lod_factor_inertia_info &last_factor_inertia() const { return lod_factor_inertia; }
    const std::vector<int>    &heat_iterations() const { return lod_heat_iterations; }
    const std::vector<double> &heat_rel_residuals() const { return lod_heat_residuals; }
    // norms of C u_H - C u_heat: the final state against the elliptic SLOD solution of solve(), and of C u_H alone
    void compare_heat_with_lod();
    const slod_error_norms &error_heat_LOD() const { return heat_lod_error; }
    const slod_error_norms &norms_LOD() const { return lod_norms; }
    // The lowest n_eig eigenpairs of A_LOD u = lambda M_LOD u after assemble_mass_matrix() (the reference has no
    // counterpart): A_LOD symmetrised (slod_lod_matrix_symmetrize), slod_lod_eigs with its documented defaults
    // (n_eig + max(4, n_eig / 2) block columns, tol 1e-10, inner tolerance 1e-12), then the eigenfunctions C x_k on the
    // fine grid (slod_lod_reconstruct_multi) and their norms (slod_compute_error_norms).
    // direct: the inner solve runs on the banded Cholesky factor of S = sym(A_LOD) - sigma M_LOD (slod_lod_matrix_combine,
    // factor_lod_matrix, slod_lod_eigs_direct); sigma must lie below the lowest eigenvalue (the factorisation fails
    // otherwise), there are no inner iteration counts, and eigen_outer_iterations() is the count of the outer ones.
    void solve_eigenproblem(const unsigned int n_eig, const bool direct = false, const double sigma = 0.0);
    // The n_eig eigenpairs NEAREST sigma, which may lie inside the spectrum: S = sym(A_LOD) - sigma M_LOD factored by LDL^T
    // (ldl; a Cholesky factor serves when S is definite) and slod_lod_eigs_shift_direct from its hashed start block, with
    // the defaults of solve_eigenproblem.  eigenvalues() are in order of distance from sigma; last_factor_inertia() gives
    // the number of eigenvalues below sigma and the growth of the factor.
    void solve_eigenproblem_near(const double sigma, const unsigned int n_eig, const bool ldl = true);
    int  eigen_outer_iterations() const { return lod_eig_outer; }
    const std::vector<double>           &eigenvalues() const { return lod_eigenvalues; }   // all block columns
    const std::vector<double>           &eigen_residuals() const { return lod_eig_residuals; }
    const std::vector<int>              &eigen_inner_iterations() const { return lod_eig_inner_iterations; } // per outer iteration
    const std::vector<slod_error_norms> &eigenfunction_norms() const { return lod_eig_norms; } // n_eig entries
    // n_steps of Newmark-beta for M u'' + A u = C^T f_h from rest (u = v = 0, M a = C^T f_h through
    // slod_lod_newmark_accel) with the load of solve(), constant in time and undamped, on the symmetrised A_LOD; after
    // assemble_mass_matrix() and assemble_and_solve_fem_problem().  One slod_lod_newmark_steps call per step (the calls
    // compose bit for bit), so that the work u^T b of every state can be formed on the host; then the final state on the
    // fine grid and its norms.  direct: the initial acceleration on the factor of M_LOD and the steps on the factor of
    // S = M + beta dt^2 sym(A_LOD) (slod_lod_newmark_accel_direct, slod_lod_newmark_steps_direct); no iteration counts.
    void solve_wave(const unsigned int n_steps, const double dt, const double beta, const double gamma, const bool direct = false);
    const std::vector<int>    &wave_iterations() const { return lod_wave_iterations; }   // per step
    const std::vector<double> &wave_rel_residuals() const { return lod_wave_residuals; } // per step
    // n_steps + 1 entries each, entry 0 the state at rest: v^T M v / 2, u^T A u / 2 and u^T b
    const std::vector<double> &wave_kinetic() const { return lod_wave_kinetic; }
    const std::vector<double> &wave_potential() const { return lod_wave_potential; }
    const std::vector<double> &wave_work() const { return lod_wave_work; }
    const slod_error_norms    &norms_wave() const { return wave_norms; }
    // solve_heat / solve_wave by a two-stage implicit Runge-Kutta scheme (SLOD_IRK_GAUSS2: order 4, SLOD_IRK_RADAU2A: order 3,
    // L-stable) with one complex solve per step: the pair of slod_lod_irk_coefficients, the complex LDL^T of
    // S = alpha sym(A_LOD) + beta M_LOD (slod_lod_factor_create_zldl, owned by this object; last_factor_info() and
    // last_factor_inertia() describe it: the range of |D|, the growth), then slod_lod_irk_heat_steps_direct in one call or
    // slod_lod_irk_wave_steps_direct once per step (the calls compose bit for bit) for the work u^T b, as solve_wave.  The
    // load is that of solve(), constant in time; the wave starts from rest, undamped, and carries no acceleration.  The
    // results are read as those of solve_heat(.., direct) and solve_wave(.., direct).
    void solve_heat_irk(const int scheme, const unsigned int n_steps, const double dt);
    void solve_wave_irk(const int scheme, const unsigned int n_steps, const double dt);
    // The steady response to the harmonic load Re(b e^{i omega t}), b the load of solve(), with the Rayleigh damping
    // C = damp_mass M + damp_stiff sym(A): (1 + i omega damp_stiff) sym(A) u + (i omega damp_mass - omega^2) M u = b for every
    // omega of the sweep in one slod_lod_harmonic_response call; after assemble_mass_matrix() and
    // assemble_and_solve_fem_problem().  Per frequency the growth of its factor, the true relative residual, the amplitude
    // (u_r^T M u_r + u_i^T M u_i)^(1/2) and the dissipated power omega u^H C u / 2, both by slod_lod_inner_multi.
    void solve_harmonic(const std::vector<double> &omegas, const double damp_mass, const double damp_stiff);
    const std::vector<double> &harmonic_growth() const { return lod_harmonic_growth; }       // per frequency
    const std::vector<double> &harmonic_residuals() const { return lod_harmonic_residuals; }
    const std::vector<double> &harmonic_amplitude() const { return lod_harmonic_amplitude; }
    const std::vector<double> &harmonic_power() const { return lod_harmonic_power; }
    // The LOD systems of all par.n_members coefficient realisations with the load f = 1, after run() (the reference
    // solves one problem, LOD.cc:976-1002): the coefficients of members 1 .. K-1, one plan over all K * n_patches bases
    // into an ensemble slab on the device, then slod_lod_matrix_ensemble, slod_lod_rhs_ensemble (one load shared),
    // slod_lod_solve_ensemble, slod_lod_reconstruct_ensemble and slod_ensemble_moments; the norms of the mean and of the
    // standard deviation (the square root of the variance, taken on the host) by slod_compute_error_norms with v = 0.
    void solve_ensemble();
    const std::vector<int>    &ensemble_iterations() const { return lod_ens_iterations; }      // per member
    const std::vector<double> &ensemble_rel_residuals() const { return lod_ens_residuals; }    // per member
    const slod_error_norms    &norms_ensemble_mean() const { return ens_mean_norms; }
    const slod_error_norms    &norms_ensemble_deviation() const { return ens_dev_norms; }
    // solve_ensemble()'s systems, symmetrised (slod_lod_matrix_symmetrize_ensemble), by CG preconditioned by the banded
    // Cholesky factor of member `member` alone, shared by all members (slod_lod_solve_ensemble_precond), and by
    // slod_lod_solve_ensemble on the same systems for the counts next to it; after solve_ensemble()
    void solve_ensemble_precond(const unsigned int member);
    const std::vector<int> &ensemble_precond_iterations() const { return lod_ens_pcg_iterations; }        // per member
    const std::vector<int> &ensemble_precond_jacobi_iterations() const { return lod_ens_pcg_jacobi; }     // per member
    // M_LOD of every member on the ensemble slab of solve_ensemble() (slod_lod_mass_matrix_ensemble, density 1); after
    // solve_ensemble()
    void assemble_mass_matrix_ensemble();
    // solve_heat(.., direct = true) for all members at once, after assemble_mass_matrix_ensemble(): S_k = M_k + theta dt A_k
    // (slod_lod_matrix_combine_ensemble), one factor object for all members (slod_lod_factor_create_ensemble; the lower
    // triangle is read, as in solve_heat) and n_steps calls of slod_lod_theta_steps_ensemble_direct with one step each
    // (the calls compose bit for bit), from u = 0 with the load of solve_ensemble().  After every step the states are
    // reconstructed and compared with the members' elliptic solutions: member k's elliptic solution is slod_lod_solve
    // on its de-interleaved matrix, so that the distances are those of solve_heat + compare_heat_with_lod of a problem
    // with member k's coefficient.  Then the moments of the final states as in solve_ensemble().  last_factor_info() is
    // the range over all members.
    void solve_heat_ensemble(const unsigned int n_steps, const double dt, const double theta);
    // [step * n_members + member]: the norms of C_k u_k - C_k u_k^heat after step + 1 steps; [member]: those of C_k u_k
    const std::vector<slod_error_norms> &error_heat_ensemble() const { return ens_heat_error; }
    const std::vector<slod_error_norms> &norms_LOD_ensemble() const { return ens_lod_norms; }
    const slod_error_norms              &norms_heat_ensemble_mean() const { return ens_heat_mean_norms; }
    const slod_error_norms              &norms_heat_ensemble_deviation() const { return ens_heat_dev_norms; }
    // solve_wave(.., direct = true) for all members at once, after assemble_mass_matrix_ensemble(): the symmetrised
    // stiffness of every member (slod_lod_matrix_symmetrize_ensemble), one factor object of M for the initial
    // acceleration (slod_lod_newmark_accel_ensemble_direct) and one of S_k = M_k + beta dt^2 sym(A_k), then n_steps calls
    // of slod_lod_newmark_steps_ensemble_direct with one step each (the calls compose bit for bit), from rest with the
    // load of solve_ensemble(), undamped.  Member k's energies are those of solve_wave of a problem with member k's
    // coefficient.  Then the final states on the fine grid and their moments as in solve_ensemble().
    // last_factor_info() is that of S, the range over all members.
    void solve_wave_ensemble(const unsigned int n_steps, const double dt, const double beta, const double gamma);
    // solve_heat_irk / solve_wave_irk for all members at once, after assemble_mass_matrix_ensemble(): the symmetrised
    // stiffness of every member (slod_lod_matrix_symmetrize_ensemble), the pair of slod_lod_irk_coefficients, one complex
    // factor object with a member per realisation (slod_lod_factor_create_zldl_ensemble with one coefficient pair;
    // last_factor_info() and last_factor_inertia() are those of member 0), then n_steps calls of
    // slod_lod_irk_heat_steps_ensemble_direct / slod_lod_irk_wave_steps_ensemble_direct with one step each (the calls
    // compose bit for bit), from u = 0 (from rest, undamped) with the load of solve_ensemble().  The results are read as
    // those of solve_heat_ensemble (error_heat_ensemble(), norms_heat_ensemble_*) and solve_wave_ensemble
    // (wave_ensemble_*, norms_wave_ensemble_*): member k's numbers are those of solve_heat_irk / solve_wave_irk of a
    // problem with member k's coefficient.
    void solve_heat_irk_ensemble(const int scheme, const unsigned int n_steps, const double dt);
    void solve_wave_irk_ensemble(const int scheme, const unsigned int n_steps, const double dt);
    // Receivers: component `component` of the FE function at the points (x, y) of the unit square, four bilinear terms each
    // (slod_lod_receivers_create on the basis slab after compute_basis_function_candidates(), or with ensemble = true on
    // the members' slabs after solve_ensemble()).  record_next(every) makes the NEXT solve_heat* / solve_wave* call record
    // them: record j holds the state after j * every steps, record 0 the entry state.  Only the loops that are one stepper
    // call (solve_heat, CG and direct, and solve_heat_irk) arm the library's record, slod_lod_time_record_arm.  solve_wave,
    // solve_wave_irk and the four ensemble loops call the stepper once per step (for the energies' work term or the
    // distances); there nothing is armed and slod_lod_observe_multi / _ensemble is queued on the same states after the
    // steps that belong to a record: the words are the same.  trace() is
    // [record][quantity (u, then v for the wave)][receiver][column (member)], on the host.
    struct ReceiverPoint
    {
      double x, y;
      int    component;
    };
    void create_receivers(const std::vector<ReceiverPoint> &points, const bool ensemble = false);
    void record_next(const unsigned int every = 1) { record_every = every; }
    const std::vector<double> &trace() const { return host_trace; }
    unsigned int trace_records() const { return trace_n_records; }
    unsigned int trace_quantities() const { return trace_nq; }
    unsigned int trace_columns() const { return trace_cols; }
    unsigned int trace_receivers() const { return n_receivers; }
    unsigned int trace_every() const { return trace_every_; }
    // Sources: unit point forces in component `component` at the points (x, y), four bilinear terms each
    // (slod_lod_sources_create on the receivers object of the same points, which is dropped afterwards; with ensemble =
    // true on the members' slabs).  drive_next(signal, n_samples) makes the NEXT solve_heat* / solve_wave* call add
    // O^T g(t) to its load: signal[j * n_sources + q] is sample j of source q, the same for every column; the theta and
    // Newmark loops read the samples 0 .. n_steps (b^k = sample k), the IRK loops the samples 2 k + i of stage i of step k.
    // solve_heat and solve_heat_irk arm the library's source once (slod_lod_time_source_arm); the six loops that call the
    // stepper once per step arm it before every call with the signal advanced by that step's samples, and the wave loops
    // form the load of the initial acceleration with slod_lod_inject_*.  quiet_load(): the loops drop the problem's own
    // load, so that a driven run is the response of the sources alone.
    void create_sources(const std::vector<ReceiverPoint> &points, const bool ensemble = false);
    void drive_next(const std::vector<double> &signal, const unsigned int n_samples)
    {
      drive_signal  = signal;
      drive_samples = n_samples;
    }
    void quiet_load(const bool quiet = true) { load_quiet = quiet; }
    // solve_harmonic for all members at once, after assemble_mass_matrix_ensemble(): the symmetrised stiffness of every
    // member (slod_lod_matrix_symmetrize_ensemble), the loads of solve_ensemble() (slod_lod_rhs_ensemble, f = 1) and one
    // slod_lod_harmonic_response_ensemble call for all (frequency, member) pairs.  Entry [frequency * n_members + member] of
    // growth, residual, amplitude and power is that of solve_harmonic of a problem with that member's coefficient: amplitude
    // and power come from slod_lod_inner_ensemble on the frequency's block of the response, which is an ensemble coarse
    // multi-vector (the call's own quantities are kept beside them).  For the frequency with the largest mean amplitude
    // the real and the imaginary block go to the fine grid (slod_lod_reconstruct_ensemble) and their moments are taken
    // as in solve_ensemble().
    void solve_harmonic_ensemble(const std::vector<double> &omegas, const double damp_mass, const double damp_stiff);
    const std::vector<double> &harmonic_ensemble_growth() const { return ens_harmonic_growth; }
    const std::vector<double> &harmonic_ensemble_residuals() const { return ens_harmonic_residuals; }
    const std::vector<double> &harmonic_ensemble_amplitude() const { return ens_harmonic_amplitude; }
    const std::vector<double> &harmonic_ensemble_power() const { return ens_harmonic_power; }
    const std::vector<double> &harmonic_ensemble_quantities() const { return ens_harmonic_quantities; } // [..][4]
    unsigned int               harmonic_ensemble_peak() const { return ens_harmonic_peak; } // the frequency reconstructed
    const slod_error_norms    &norms_harmonic_ensemble_real_mean() const { return ens_harmonic_norms[0]; }
    const slod_error_norms    &norms_harmonic_ensemble_real_deviation() const { return ens_harmonic_norms[1]; }
    const slod_error_norms    &norms_harmonic_ensemble_imag_mean() const { return ens_harmonic_norms[2]; }
    const slod_error_norms    &norms_harmonic_ensemble_imag_deviation() const { return ens_harmonic_norms[3]; }
    // solve_eigenproblem(.., direct = true) for all members at once, after assemble_mass_matrix_ensemble(): the symmetrised
    // stiffness of every member, S_k = sym(A_k) - sigma M_k (sigma = 0: sym(A_k) itself), one factor object for all members
    // and slod_lod_eigs_ensemble_direct with the defaults of solve_eigenproblem.  Member k's eigenvalues, residuals and
    // outer count are those of solve_eigenproblem(.., true, sigma) of a problem with member k's coefficient.
    // last_factor_info() is the range over all members.
    void solve_eigenproblem_ensemble(const unsigned int n_eig, const double sigma = 0.0);
    // solve_eigenproblem_near for all members at once, one sigma for all (slod_lod_factor_create_ldl_ensemble,
    // slod_lod_eigs_shift_ensemble_direct); factor_inertia_ensemble()[k] is member k's inertia and growth.
    void solve_eigenproblem_ensemble_near(const double sigma, const unsigned int n_eig, const bool ldl = true);
    const std::vector<slod_lod_factor_inertia_info> &factor_inertia_ensemble() const { return ens_factor_inertia; }
    // [member * n_block + column], n_block = eigen_ensemble_block(); [member]
    const std::vector<double> &eigenvalues_ensemble() const { return ens_eigenvalues; }
    const std::vector<double> &eigen_residuals_ensemble() const { return ens_eig_residuals; }
    const std::vector<int>    &eigen_outer_iterations_ensemble() const { return ens_eig_outer; }
    int                        eigen_ensemble_block() const { return ens_eig_block; }
    // [step * n_members + member], step = 0 .. n_steps, step 0 the state at rest: v^T M v / 2, u^T A u / 2 and u^T b
    const std::vector<double> &wave_ensemble_kinetic() const { return ens_wave_kinetic; }
    const std::vector<double> &wave_ensemble_potential() const { return ens_wave_potential; }
    const std::vector<double> &wave_ensemble_work() const { return ens_wave_work; }
    const slod_error_norms    &norms_wave_ensemble_mean() const { return ens_wave_mean_norms; }
    const slod_error_norms    &norms_wave_ensemble_deviation() const { return ens_wave_dev_norms; }
    // After assemble_global_matrix(), when the coefficient of the problem class has changed in part of the domain (the
    // reference has no counterpart): re-samples it (slod_update_coefficient finds the patches that see a changed fine
    // element), rebuilds those patches in place on the device slab (slod_plan_create_dirty), recomputes the entries of
    // A_LOD with such a row or column (slod_lod_matrix_update), those of M_LOD if assemble_mass_matrix() has run
    // (slod_lod_mass_matrix_update), and brings Patch::basis_function of the rebuilt patches up to date.  Returns the
    // number of rebuilt patches.  solve() and the other consumers then see the new coefficient.
    unsigned int refresh_after_coefficient_change();
    // values of the block rows of A_LOD (the layout of slod_lod_matrix) and u_H of the last solve(), copied from the device
    std::vector<double> lod_matrix_values() const;
    std::vector<double> lod_solution() const;
    const slod_error_norms &error_LOD_FEMh() const { return lod_fem_error; }
    // the same norms of u_h alone (the denominators of relative errors)
    const slod_error_norms &norms_FEMh() const { return fem_norms; }
    // The coarse FEM(H) problem with f = 1 (the coarse block of assemble_and_solve_fem_problem, LOD.cc:1103-1237,
    // which the reference runs for spacedim == 2 only and marks TODO; here for both problem classes), after
    // assemble_and_solve_fem_problem(): the coefficient at the Gauss points of the coarse cells
    // (assemble_stiffness_coarse), load vector, solve, FETools::interpolate onto the fine space and
    // error_FEMH_FEMh.difference(u_h, interpolated) (LOD.cc:1206-1208).
    void assemble_and_solve_coarse_fem_problem();
    const slod_error_norms &error_FEMH_FEMh() const { return femH_fem_error; }
    // fem_coarse_solution_interpolated (LOD.cc:1199-1204) on the fine grid, [(NE+1)^2][spacedim] lexicographic,
    // component-minor; copied from the device on every call
    std::vector<double> fem_coarse_solution_interpolated() const;

  protected:
    void make_fe();
    void make_grid();
    void create_patches();
    void create_mesh_for_patch(Patch<dim> &current_patch);
    void initialize_patches();
    void compute_basis_function_candidates();
    virtual void create_random_problem_coefficients() {}
    // Replaces the coefficient evaluation inside the virtual assemble_stiffness
    // (Diffusion.h:154, Elasticity.h:208-209): fill `values` with field `field` (0 = alpha or
    // lambda, 1 = mu) at the quadrature points, index ((ey*NE + ex)*4 + q).
    virtual void coefficients_at_quadrature_points(const unsigned int          field,
                                                   const std::vector<Point<dim>> &points,
                                                   std::vector<double> &        values) = 0;
    // The same for realisation `member` >= 1 of an ensemble; a problem class that can draw further realisations of
    // its coefficient overrides it.
    virtual void member_coefficients_at_quadrature_points(const unsigned int member, const unsigned int,
                                                          const std::vector<Point<dim>> &, std::vector<double> &)
    {
      throw std::runtime_error("this problem class has no coefficient for ensemble member " + std::to_string(member));
    }
    // assemble_stiffness(patch_stiffness_matrix, dummy, dh_fine_patch, empty_constraints)
    // (LOD.cc:440-444) for one patch: the unconstrained 9-point block stencil
    // stencil[node][dir][a][b] computed on the GPU.
    void assemble_stiffness(const unsigned int patch_id, std::vector<double> &stencil);

    const LODParameters<dim, spacedim> &par;
    std::vector<Patch<dim>>             patches;
    std::pair<unsigned int, unsigned int> locally_owned_patches{0, 0}; // [begin, end)
    unsigned int                          this_mpi_process = 0, n_mpi_processes = 1;
    slod_handle *                         handle = nullptr;
    double                                last_build_seconds = 0.0;

    // device arrays of the global steps (freed by the destructor)
    std::vector<void *> device_arrays;
    std::size_t         basis_stride = 0;
    double             *d_basis = nullptr, *d_premult = nullptr, *d_lod_values = nullptr;
    uint32_t           *d_lod_cols = nullptr;
    double             *d_fem_rhs = nullptr, *d_fem_solution = nullptr, *d_lod_u = nullptr;
    double             *d_fem_coarse_solution = nullptr, *d_fem_coarse_interpolated = nullptr;
    slod_error_norms    lod_fem_error{}, fem_norms{}, femH_fem_error{};
    // assemble_mass_matrix, solve_heat
    double             *d_lod_damping = nullptr; // assemble_damping_matrix
    unsigned int        lod_damping_zero_rows = 0;
    double             *d_lod_mass = nullptr, *d_heat_rhs = nullptr, *d_heat_u = nullptr, *d_heat_fine = nullptr;
    std::vector<int>    lod_heat_iterations;
    std::vector<double> lod_heat_residuals;
    slod_error_norms    heat_lod_error{}, lod_norms{};
    // solve_eigenproblem: the symmetrised stiffness, the block X and the reconstructed eigenfunctions
    double                       *d_lod_sym = nullptr, *d_eig_x = nullptr, *d_eig_fine = nullptr;
    std::vector<double>           lod_eigenvalues, lod_eig_residuals;
    std::vector<int>              lod_eig_inner_iterations;
    int                           lod_eig_outer = 0;
    std::vector<slod_error_norms> lod_eig_norms;
    // solve_wave: u, v, a and the load (4 coarse vectors), the final state on the fine grid
    double             *d_wave_state = nullptr, *d_wave_fine = nullptr;
    std::vector<int>    lod_wave_iterations;
    std::vector<double> lod_wave_residuals, lod_wave_kinetic, lod_wave_potential, lod_wave_work;
    slod_error_norms    wave_norms{};
    // solve_harmonic: the load and the two planes of the response (1 + 2 n_freq coarse vectors)
    double             *d_harmonic = nullptr;
    std::size_t         harmonic_capacity = 0;
    std::vector<double> lod_harmonic_growth, lod_harmonic_residuals, lod_harmonic_amplitude, lod_harmonic_power;
    // factor_lod_matrix: the factors this object owns, the matrix S of a direct time loop
    std::vector<slod_lod_factor *> factors;
    slod_lod_factor_info           lod_factor_info{};
    slod_lod_factor_inertia_info   lod_factor_inertia{};
    double                        *d_lod_shifted = nullptr;
    // factor_for_reuse, solve_precond, solve_ensemble_precond
    slod_lod_factor *reuse_factor = nullptr;
    double          *d_pcg_u = nullptr, *d_ens_pcg_u = nullptr;
    int              lod_pcg_iterations = 0, lod_pcg_jacobi_iterations = 0;
    std::vector<int> lod_ens_pcg_iterations, lod_ens_pcg_jacobi;
    // solve_multi: fine load vectors and reconstructions, field k at + k * fine_size
    double                       *d_multi_fem_rhs = nullptr, *d_multi_fine = nullptr;
    std::vector<int>              lod_multi_iterations;
    std::vector<double>           lod_multi_residuals;
    std::vector<slod_error_norms> lod_multi_fem_error;
    // solve_ensemble
    std::vector<int>    lod_ens_iterations;
    std::vector<double> lod_ens_residuals;
    slod_error_norms    ens_mean_norms{}, ens_dev_norms{};
    // what solve_ensemble leaves for the ensemble time loop: slab, matrices, columns, coarse loads; then M and S
    std::size_t ens_stride = 0, ens_member_stride = 0;
    double     *d_ens_basis = nullptr, *d_ens_values = nullptr, *d_ens_rhs = nullptr, *d_ens_mass = nullptr, *d_ens_shifted = nullptr;
    uint32_t   *d_ens_cols = nullptr;
    std::vector<slod_error_norms> ens_heat_error, ens_lod_norms;
    slod_error_norms              ens_heat_mean_norms{}, ens_heat_dev_norms{};
    // solve_wave_ensemble: the symmetrised stiffness of the members
    double             *d_ens_sym = nullptr;
    std::vector<double> ens_wave_kinetic, ens_wave_potential, ens_wave_work;
    slod_error_norms    ens_wave_mean_norms{}, ens_wave_dev_norms{};
    // solve_harmonic_ensemble
    std::vector<double> ens_harmonic_growth, ens_harmonic_residuals, ens_harmonic_amplitude, ens_harmonic_power, ens_harmonic_quantities;
    unsigned int        ens_harmonic_peak = 0;
    slod_error_norms    ens_harmonic_norms[4] = {};
    // solve_eigenproblem_ensemble
    std::vector<double> ens_eigenvalues, ens_eig_residuals;
    std::vector<int>    ens_eig_outer;
    int                 ens_eig_block = 0;
    std::vector<slod_lod_factor_inertia_info> ens_factor_inertia;
    // the bodies of solve_eigenproblem / _near and of their ensemble forms: near orders the pairs by distance from sigma
    void eigenproblem(const unsigned int n_eig, const bool direct, const double sigma, const bool near, const bool ldl);
    void eigenproblem_ensemble(const unsigned int n_eig, const double sigma, const bool near, const bool ldl);
    // mean and standard deviation of n_members fine fields: slod_ensemble_moments, the square root on the host, the norms
    void ensemble_moment_norms(const double *d_fine, double *d_mean, double *d_var, slod_error_norms &mean, slod_error_norms &dev);
    // the members' elliptic solutions on the fine grid, [member][fine_size], and their norms (ens_lod_norms): the
    // reference of the ensemble heat loops
    void ensemble_elliptic_solutions(double *d_ell_fine);
    // sym(A_k) of every member into d_ens_sym and the complex factor of the scheme's step matrices, a member per realisation
    slod_lod_factor *factor_lod_irk_ensemble(const int scheme, const int order, const double dt);
    // create_receivers / record_next.  record_open: when a record is pending, the trace of a loop of n_steps on `columns`
    // columns (DEVICE, zeroed) and true; record_arm: before a stepper call that runs the whole loop; record_state: after
    // `steps_done` one-step calls, the product on (d_u, d_v) if that state belongs to a record; record_close: the trace to the host.
    slod_lod_receivers *receivers = nullptr, *ens_receivers = nullptr;
    unsigned int        n_receivers = 0, record_every = 0, trace_every_ = 1, trace_n_records = 0, trace_nq = 0, trace_cols = 0;
    bool                trace_open = false, trace_ensemble = false;
    double             *d_trace = nullptr;
    std::size_t         d_trace_size = 0;
    std::vector<double> host_trace;
    bool record_open(const unsigned int n_steps, const unsigned int columns, const bool has_v, const bool ensemble);
    void record_arm(const unsigned int n_steps);
    void record_state(const unsigned int steps_done, const double *d_u, const double *d_v);
    void record_close();
    // create_sources / drive_next / quiet_load.  make_receivers: the receivers object of a set of points.  source_open: when
    // a signal is pending (one-shot), it goes to the device replicated over `columns` columns, checked against the
    // `needed` samples of the loop, and true; source_arm: before a stepper call, from sample `first` on; source_load: the
    // load d_load + O^T g(sample 0) of the initial acceleration in d_out (d_load when nothing is open); own_load: d_load or,
    // quiet, NULL.
    slod_lod_sources   *sources = nullptr, *ens_sources = nullptr;
    unsigned int        n_sources = 0, drive_samples = 0, drive_samples_open = 0, drive_cols = 0;
    bool                drive_open = false, drive_ensemble = false, load_quiet = false;
    std::vector<double> drive_signal;
    double             *d_signal = nullptr, *d_wave_load0 = nullptr;
    std::size_t         d_signal_size = 0;
    slod_lod_receivers *make_receivers(const std::vector<ReceiverPoint> &points, const bool ensemble, const char *who);
    bool          source_open(const unsigned int needed, const unsigned int columns, const bool ensemble);
    void          source_arm(const unsigned int first);
    const double *source_load(const double *d_load, double *d_out);
    const double *own_load(const double *d_load) const { return load_quiet ? nullptr : d_load; }

    void check(const int status, const char *what) const;
    std::vector<Point<dim>> fine_quadrature_points() const;
    template <typename T>
    T *device_alloc(std::size_t n);
  };
} // namespace slod

#endif
