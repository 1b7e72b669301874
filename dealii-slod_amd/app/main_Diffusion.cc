// Counterpart of reference app/main_Diffusion.cc for the basis-construction path:
//   main_Diffusion [n_global_refinements n_subdivisions oversampling stabilize [dump.bin]] [--compare] [--coarse] [--loads K]
//                  [--heat STEPS DT] [--eigs K] [--shift SIGMA] [--wave STEPS DT] [--direct] [--irk gauss|radau] [--ensemble K] [--perturb K]
//                  [--reuse-factor] [--precond-member J]
//                  [--member K] [--ldl] [--harmonic K W0 W1 [--damping DM DS]] (with --ensemble: per member)
//                  [--sponge WIDTH SIGMA_MAX]
//                  [--receiver X Y [C]]... [--record-every M]
//                  [--source X Y [C]]... [--ricker F0 T0 [AMP]] [--quiet-load]
// prints the reference's patch summary (LOD.cc:237-242) and a digest of the basis; with a
// file name it dumps, per patch, phi and psi in patch-lexicographic order (parity tests).
// --compare (anywhere on the command line): after run(), the rest of the reference run() -- global
// matrix, fine FEM solve (f = 1), LOD solve, compare_lod_with_fem -- and the "SLOD vs reference FEM(h)"
// errors (LOD.cc:1462-1463) in L2, H1, Linfty and the energy norm.
// --coarse implies --compare and adds the coarse FEM(H) problem (LOD.cc:1103-1237): its table "FEM(H) vs
// reference FEM(h)" comes before the SLOD table, the reference's order (LOD.cc:1458-1465).
// --loads K: the LOD system for the K loads f_k = sin(k pi x) sin(pi y), k = 1 .. K, in one multi-vector solve
// (slod_lod_solve_multi); one line per load with its iterations and relative residual, with --compare also the
// L2 and energy error against the fine FEM solution of that load.
// --heat STEPS DT: the heat flow  M u' + A u = C^T f  (f = 1, constant in time) from u = 0 by STEPS backward Euler steps
// of size DT on the LOD space (slod_lod_theta_steps): one line per step with its iterations and relative residual, then
// the table "SLOD heat flow at T = STEPS DT vs elliptic SLOD solution", which shrinks as STEPS DT grows.
// --eigs K: the K lowest eigenpairs of  A_LOD u = lambda M_LOD u  (A_LOD symmetrised, slod_lod_eigs with its defaults): one
// line per pair with its eigenvalue and residual, the outer and inner iteration counts, and the fine-grid L2 norm of
// every reconstructed eigenfunction.
// --eigs K --direct [--shift SIGMA]: the same pairs with the inner solve on the banded Cholesky factor of
// S = sym(A_LOD) - SIGMA M_LOD (slod_lod_eigs_direct; SIGMA below the lowest eigenvalue, default 0): the eigenvalue lines,
// "eigensolver: outer iterations = N, direct", the factor line in place of the inner iteration counts, the norms.
// --eigs K --direct --shift SIGMA --ldl: SIGMA may lie inside the spectrum.  S is factored by the banded LDL^T without
// pivoting (slod_lod_factor_create_ldl) and the K pairs NEAREST SIGMA are computed (slod_lod_eigs_shift_direct), printed in
// order of distance from SIGMA.  The factor line reads "factor: n = .., half bandwidth = .., bytes = .., LDL^T, n_negative
// = .. (eigenvalues below sigma), growth = ..".  With --ensemble K the same per member ("member K factor: n_negative = ..,
// growth = .."), then the mean and standard deviation of n_negative and of each eigenvalue over the members.
// --ensemble K --eigs N --direct: after the lines of --ensemble, the N lowest pairs of every member on one factor object
// (slod_lod_eigs_ensemble_direct): the factor line (pivots over all members), per member "member K eigenvalue J = ..,
// residual = .." and "member K eigensolver: outer iterations = .., direct", the numbers of a --member K --eigs N --direct
// run, then per eigenvalue "eigenvalue J over the ensemble of K: mean = .., standard deviation = ..".
// --wave STEPS DT: the wave equation  M u'' + A u = C^T f  (f = 1, constant in time, A_LOD symmetrised) from rest by STEPS
// steps of the trapezoidal rule (Newmark gamma = 1/2, beta = 1/4, slod_lod_newmark_steps): one line per step with its
// iterations, relative residual, kinetic and potential energy and the work u^T b (kinetic + potential = work from rest
// under a constant load), then the fine-grid L2 norm of the reconstructed final state.
// --harmonic K W0 W1 [--damping DM DS]: the steady response to the load Re(C^T f e^{i omega t}) (f = 1, A_LOD symmetrised) at K
// frequencies evenly spaced in [W0, W1] with the Rayleigh damping C = DM M + DS A (default 0 0), by one
// slod_lod_harmonic_response call (a complex symmetric banded LDL^T per frequency); one line per frequency, "harmonic J:
// omega = .., growth = .., relative residual = .., amplitude = .., power = ..": the growth of the factor, the true residual,
// (u^H M u)^(1/2) and the dissipated power omega u^H C u / 2.
// --ensemble K --harmonic F W0 W1 [--damping DM DS]: after the lines of --ensemble, the same sweep for every member in one
// slod_lod_harmonic_response_ensemble call: "harmonic J member M: omega = .., growth = .., relative residual = .., amplitude
// = .., power = ..", the numbers of the "harmonic J" line of a --member M --harmonic run; per frequency "harmonic J amplitude
// over the ensemble of K: mean = .., standard deviation = .."; then for the frequency with the largest mean amplitude the L2
// norms of the mean and of the standard deviation of the real and of the imaginary part on the fine grid.
// --sponge WIDTH SIGMA_MAX (with --wave STEPS DT [--direct] [--irk gauss|radau] and with --harmonic; not with --ensemble): a
// sponge layer, the damping matrix D = C^T M_sigma C with sigma = SIGMA_MAX max(0, 1 - d / WIDTH)^2 per fine element (d the
// distance of its centre from the rim), joins the model: M u'' + D u' + A u = C^T f, and S(omega) gains i omega D.  Prints
// "sponge: width = .., sigma_max = .., zero coarse rows of D = .." ahead of the loop; the per-step and per-frequency lines
// keep their format, and the harmonic power includes u^H D u.
// --heat STEPS DT --irk gauss|radau, --wave STEPS DT --irk gauss|radau: the time loop by a two-stage implicit Runge-Kutta
// scheme (Gauss-Legendre, order 4; Radau IIA, order 3, L-stable) with one complex solve per step on the complex LDL^T of its
// step matrix (slod_lod_irk_coefficients, slod_lod_factor_create_zldl, slod_lod_irk_heat_steps_direct /
// slod_lod_irk_wave_steps_direct; A_LOD symmetrised for both): the lines of --direct, the factor line with the range of |D|,
// and behind it "factor: complex LDL^T of the SCHEME step, growth = ..".
// --receiver X Y [C] (repeatable), --record-every M: with any flavour of --heat / --wave (CG, --direct, --irk, each with
// --ensemble K or --member K) component C (default 0) of the solution at the point (X, Y) of the unit square is recorded
// inside the time loop (LOD::create_receivers, LOD::record_next): after the loop one line per record, receiver and member,
// "heat|wave receiver Q member K record J: t = .., u = ..[, v = ..]", record J the state after J * M steps, record 0 the
// entry state.  With --ensemble K the ensemble loop records and the lines of member K are those of a --member K run.
// The argument after "--receiver X Y" is taken as C whenever it is a plain non-negative integer, so the positional
// arguments go before the first --receiver (or give C).  --receiver with fewer than two arguments, or without --heat or
// --wave, is refused.  Of these loops only --heat without --ensemble runs the library's armed record
// (slod_lod_time_record_arm); the others step one call at a time and observe the same states (LOD.h).
// --source X Y [C] (repeatable) with --ricker F0 T0 [AMP]: a unit point force in component C at (X, Y), scaled in time by the
// Ricker wavelet AMP (1 - 2 a) exp(-a), a = (pi F0 (t - T0))^2, drives every --heat / --wave loop (CG, --direct, --irk, each
// with --ensemble K or --member K) through LOD::create_sources and LOD::drive_next: the source adds to the loop's load.  The
// wavelet is sampled where the loop reads its load: at t_k = k DT, and with --irk at the stage times t_k + c_i DT.
// --quiet-load drops the problem's own load (f = 1), so that the --receiver lines are the response of the sources alone.
// --source without --ricker (or the reverse), or without --heat or --wave, is refused.
// --direct: the time loops of --heat and --wave run on a banded Cholesky factor of their matrix S instead of CG
// (slod_lod_factor_create once, slod_lod_theta_steps_direct / slod_lod_newmark_steps_direct): one line "factor: n = ..,
// half bandwidth = .., bytes = .., pivots in [.., ..]" per loop, then the same per-step lines without iterations and
// residuals (the heat loop has none left: "heat step K").
// --ensemble K: K realisations of the run's random coefficient (member 0 is the coefficient of a run without the flag,
// the others are drawn after it), f = 1: one plan for all K * patches bases, then the K LOD systems in one call per step
// (slod_lod_matrix_ensemble, _rhs_, _solve_, _reconstruct_ensemble, slod_ensemble_moments): one line per member with its
// iterations and relative residual, then the fine-grid L2 norms of the mean and of the standard deviation.
// --ensemble K --heat STEPS DT --direct: after the lines above, the heat flow of every member on banded Cholesky factors,
// one per member in one factor object (slod_lod_mass_matrix_ensemble, slod_lod_matrix_combine_ensemble,
// slod_lod_factor_create_ensemble, slod_lod_theta_steps_ensemble_direct): the factor line (pivots over all members), one
// line "member K heat step J: L2 distance = .., energy distance = .." per member and step with the distance to that
// member's elliptic solution, then the L2 norms of the mean and of the standard deviation of the final states.  Without
// --direct the two flags act independently, as before.
// --ensemble K --wave STEPS DT --direct: after the lines above, the wave of every member from rest by the trapezoidal rule on
// banded Cholesky factors (slod_lod_matrix_symmetrize_ensemble, one factor object of M and one of S,
// slod_lod_newmark_accel_ensemble_direct, slod_lod_newmark_steps_ensemble_direct): the factor line of S (pivots over all
// members), one line "member K wave step J: kinetic = .., potential = .., work = .." per member and step, the numbers of
// the "wave step J" line of a --member K --wave STEPS DT --direct run, then the L2 norms of the mean and of the standard
// deviation of the final states.  Without --direct the two flags act independently.
// --ensemble K --heat STEPS DT --irk gauss|radau, --ensemble K --wave STEPS DT --irk gauss|radau: after the lines above, the
// same loops of every member by the two-stage scheme on one complex factor object with a member per realisation
// (slod_lod_factor_create_zldl_ensemble, slod_lod_irk_heat_steps_ensemble_direct / slod_lod_irk_wave_steps_ensemble_direct):
// the complex factor lines of member 0, "member K irk heat step J: L2 distance = .., energy distance = .." or "member K irk
// wave step J: kinetic = .., potential = .., work = ..", the numbers of a --member K .. --irk run, then one line "SLOD irk
// heat|wave ensemble of K at T = ..: L2 norm of the mean = .., of the standard deviation = ..".
// --member K: a run without --ensemble on the coefficient that is member K of an ensemble run (K fields are drawn and
// dropped before the problem draws its own).
// --perturb K: a local coefficient change after everything else.  K cells of the coefficient's 2^r x 2^r grid, picked by a
// fixed linear congruential generator, flip between min and max; the basis and A_LOD are refreshed in place
// (refresh_after_coefficient_change: only the patches that see a changed fine element, only the matrix entries with such a
// row or column) and the system is solved (f = 1).  Then a second problem with the changed coefficient is built from
// scratch.  Prints the dirty count "D of NP", max |A_refresh - A_rebuild| over the block rows and max |u_refresh -
// u_rebuild| of the coarse solutions, each with the scale it is relative to.
// --perturb K --reuse-factor: sym(A_LOD) is factored before the flip (banded Cholesky), and after the refresh the refreshed
// system is also solved by CG preconditioned by that stale factor (slod_lod_solve_multi_precond).  After the lines of
// --perturb: "stale factor as preconditioner: dirty patches = D of NP, PCG iterations = I, Jacobi-CG iterations = J" (J: the
// recurrence of slod_lod_solve_multi on the same symmetrised system) and max |u_pcg - u_rebuild| with its scale.
// --ensemble K --precond-member J: after the lines of --ensemble, the symmetrised systems of all members by CG
// preconditioned by the factor of member J alone (slod_lod_solve_ensemble_precond): per member "member k: PCG iterations
// = I, Jacobi-CG iterations = J" (J: slod_lod_solve_ensemble on the same systems).
#include "../host/Diffusion.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace slod;

class Problem : public DiffusionProblem<2, 1>
{
public:
  using DiffusionProblem<2, 1>::DiffusionProblem;
  void dump(const char *file) const
  {
    FILE *f = std::fopen(file, "wb");
    if (!f)
      throw std::runtime_error("cannot open dump file");
    for (const auto &p : get_patches())
      {
        const std::size_t   n = p.basis_function[0].size();
        std::vector<double> lex(n);
        for (int which = 0; which < 2; ++which)
          {
            const auto &v = which ? p.basis_function_premultiplied[0] : p.basis_function[0];
            for (std::size_t i = 0; i < n; ++i)
              lex[p.dealii_to_lexicographic[i]] = v[i];
            std::fwrite(lex.data(), sizeof(double), n, f);
          }
      }
    std::fclose(f);
  }
};

// f_k = sin(k pi x) sin(pi y)
class SineLoad : public Function<2>
{
public:
  explicit SineLoad(int k)
    : k(k)
  {}
  double value(const Point<2> &p, const unsigned int = 0) const override
  {
    return std::sin(k * M_PI * p(0)) * std::sin(M_PI * p(1));
  }

private:
  int k;
};

static void print_factor(const slod_lod_factor_info &f)
{
  std::printf("factor: n = %d, half bandwidth = %d, bytes = %llu, pivots in [%.6e, %.6e]\n", f.n, f.half_bandwidth,
              (unsigned long long)f.bytes, f.min_pivot, f.max_pivot);
}

static void print_irk_factor(const char *scheme, const slod_lod_factor_info &f, const slod_lod_factor_inertia_info &i)
{
  print_factor(f);
  std::printf("factor: complex LDL^T of the %s step, growth = %.6e\n", scheme, i.norm_factor / i.norm_matrix);
}

static void print_ldl_factor(const slod_lod_factor_info &f, const slod_lod_factor_inertia_info &i)
{
  std::printf("factor: n = %d, half bandwidth = %d, bytes = %llu, LDL^T, n_negative = %d (eigenvalues below sigma), growth = %.6e\n",
              f.n, f.half_bandwidth, (unsigned long long)f.bytes, i.n_negative, i.norm_factor / i.norm_matrix);
}

// The trace of the receivers after a time loop: one line per record, receiver and member, "<what> receiver Q member K record
// J: t = .., u = ..[, v = ..]"; a run without --ensemble prints its --member as K, so that the lines of --ensemble K are those
// of K runs with --member.
template <typename P>
static void print_trace(const P &problem, const char *what, const double dt, const int first_member)
{
  const unsigned int nr = problem.trace_receivers(), nc = problem.trace_columns(), nq = problem.trace_quantities();
  const std::vector<double> &t = problem.trace();
  for (unsigned int j = 0; j < problem.trace_records(); ++j)
    for (unsigned int q = 0; q < nr; ++q)
      for (unsigned int c = 0; c < nc; ++c)
        {
          const double time = (double)(j * problem.trace_every()) * dt;
          std::printf("%s receiver %u member %u record %u: t = %.12e, u = %.12e", what, q, (unsigned int)first_member + c, j, time,
                      t[(((std::size_t)j * nq + 0) * nr + q) * nc + c]);
          if (nq == 2)
            std::printf(", v = %.12e", t[(((std::size_t)j * nq + 1) * nr + q) * nc + c]);
          std::printf("\n");
        }
}

// sample mean and unbiased standard deviation, summed in ascending order
// AMP (1 - 2 a) exp(-a), a = (pi f0 (t - t0))^2
static double ricker(const double t, const double f0, const double t0, const double amp)
{
  const double x = M_PI * f0 * (t - t0), a = x * x;
  return amp * (1.0 - 2.0 * a) * std::exp(-a);
}

static void mean_and_deviation(const std::vector<double> &x, double &mean, double &dev)
{
  mean = 0.0;
  for (const double v : x)
    mean += v;
  mean /= (double)x.size();
  double var = 0.0;
  for (const double v : x)
    var += (v - mean) * (v - mean);
  dev = std::sqrt(x.size() > 1 ? var / (double)(x.size() - 1) : 0.0);
}

int main(int argc_all, char **argv_all)
{
  // --compare and --coarse are taken out wherever they stand; the positional arguments keep their meaning
  bool               compare = false, coarse = false, direct = false, ldl = false;
  int                n_harmonic = 0;
  double             harmonic_w0 = 0.0, harmonic_w1 = 0.0, damp_mass = 0.0, damp_stiff = 0.0;
  double             sponge_width = 0.0, sponge_max = 0.0; // --sponge WIDTH SIGMA_MAX
  int                n_loads = 0, heat_steps = 0, n_eigs = 0, wave_steps = 0, n_members = 0, n_perturb = 0, member = 0, precond_member = -1;
  bool               reuse_factor = false;
  double             heat_dt = 0.0, wave_dt = 0.0, shift = 0.0;
  int                irk = -1; // --irk gauss | radau: SLOD_IRK_GAUSS2, SLOD_IRK_RADAU2A
  const char        *irk_name = "";
  std::vector<char *> args;
  std::vector<Problem::ReceiverPoint> receivers; // --receiver X Y [C], repeatable
  int                record_every = 1;           // --record-every M
  std::vector<Problem::ReceiverPoint> sources;   // --source X Y [C], repeatable
  bool               have_ricker = false, quiet_load = false; // --ricker F0 T0 [AMP], --quiet-load
  double             ricker_f0 = 0.0, ricker_t0 = 0.0, ricker_amp = 1.0;
  for (int i = 0; i < argc_all; ++i)
    if (i > 0 && !std::strcmp(argv_all[i], "--compare"))
      compare = true;
    else if (i > 0 && !std::strcmp(argv_all[i], "--receiver"))
      {
        if (i + 2 >= argc_all)
          {
            std::fprintf(stderr, "--receiver takes X Y [C]\n");
            return 1;
          }
        Problem::ReceiverPoint p{std::atof(argv_all[i + 1]), std::atof(argv_all[i + 2]), 0};
        i += 2;
        // the component, when the next argument is a plain non-negative integer
        if (i + 1 < argc_all && argv_all[i + 1][0] != '\0' && std::strspn(argv_all[i + 1], "0123456789") == std::strlen(argv_all[i + 1]))
          p.component = std::atoi(argv_all[++i]);
        receivers.push_back(p);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--source"))
      {
        if (i + 2 >= argc_all)
          {
            std::fprintf(stderr, "--source takes X Y [C]\n");
            return 1;
          }
        Problem::ReceiverPoint p{std::atof(argv_all[i + 1]), std::atof(argv_all[i + 2]), 0};
        i += 2;
        if (i + 1 < argc_all && argv_all[i + 1][0] != '\0' && std::strspn(argv_all[i + 1], "0123456789") == std::strlen(argv_all[i + 1]))
          p.component = std::atoi(argv_all[++i]);
        sources.push_back(p);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--ricker") && i + 2 < argc_all)
      {
        have_ricker = true;
        ricker_f0   = std::atof(argv_all[++i]);
        ricker_t0   = std::atof(argv_all[++i]);
        // the amplitude, when the next argument is a number and no flag
        if (i + 1 < argc_all && std::strncmp(argv_all[i + 1], "--", 2) != 0)
          {
            char        *end = nullptr;
            const double amp = std::strtod(argv_all[i + 1], &end);
            if (end != argv_all[i + 1] && *end == '\0')
              {
                ricker_amp = amp;
                ++i;
              }
          }
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--quiet-load"))
      quiet_load = true;
    else if (i > 0 && !std::strcmp(argv_all[i], "--record-every") && i + 1 < argc_all)
      record_every = std::atoi(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--coarse"))
      compare = coarse = true;
    else if (i > 0 && !std::strcmp(argv_all[i], "--direct"))
      direct = true;
    else if (i > 0 && !std::strcmp(argv_all[i], "--ldl"))
      ldl = true;
    else if (i > 0 && !std::strcmp(argv_all[i], "--irk") && i + 1 < argc_all)
      {
        irk_name = argv_all[++i];
        irk      = !std::strcmp(irk_name, "gauss") ? SLOD_IRK_GAUSS2 : !std::strcmp(irk_name, "radau") ? SLOD_IRK_RADAU2A : -2;
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--loads") && i + 1 < argc_all)
      n_loads = std::atoi(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--heat") && i + 2 < argc_all)
      {
        heat_steps = std::atoi(argv_all[++i]);
        heat_dt    = std::atof(argv_all[++i]);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--eigs") && i + 1 < argc_all)
      n_eigs = std::atoi(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--shift") && i + 1 < argc_all)
      shift = std::atof(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--wave") && i + 2 < argc_all)
      {
        wave_steps = std::atoi(argv_all[++i]);
        wave_dt    = std::atof(argv_all[++i]);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--harmonic") && i + 3 < argc_all)
      {
        n_harmonic  = std::atoi(argv_all[++i]);
        harmonic_w0 = std::atof(argv_all[++i]);
        harmonic_w1 = std::atof(argv_all[++i]);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--damping") && i + 2 < argc_all)
      {
        damp_mass  = std::atof(argv_all[++i]);
        damp_stiff = std::atof(argv_all[++i]);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--sponge") && i + 2 < argc_all)
      {
        sponge_width = std::atof(argv_all[++i]);
        sponge_max   = std::atof(argv_all[++i]);
      }
    else if (i > 0 && !std::strcmp(argv_all[i], "--ensemble") && i + 1 < argc_all)
      n_members = std::atoi(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--member") && i + 1 < argc_all)
      member = std::atoi(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--perturb") && i + 1 < argc_all)
      n_perturb = std::atoi(argv_all[++i]);
    else if (i > 0 && !std::strcmp(argv_all[i], "--reuse-factor"))
      reuse_factor = true;
    else if (i > 0 && !std::strcmp(argv_all[i], "--precond-member") && i + 1 < argc_all)
      precond_member = std::atoi(argv_all[++i]);
    else
      args.push_back(argv_all[i]);
  const int argc = (int)args.size();
  char    **argv = args.data();
  try
    {
      if (irk == -2)
        throw std::runtime_error("--irk takes gauss or radau");
      if (record_every < 1)
        throw std::runtime_error("--record-every takes M >= 1");
      if (!receivers.empty() && heat_steps <= 0 && wave_steps <= 0)
        throw std::runtime_error("--receiver records inside a time loop: give --heat STEPS DT or --wave STEPS DT");
      if (sources.empty() != !have_ricker)
        throw std::runtime_error("--source X Y [C] and --ricker F0 T0 [AMP] come together");
      if (!sources.empty() && heat_steps <= 0 && wave_steps <= 0)
        throw std::runtime_error("--source drives a time loop: give --heat STEPS DT or --wave STEPS DT");
      const bool sponge = sponge_width != 0.0 || sponge_max != 0.0;
      if (sponge && (!(sponge_width > 0.0) || !(sponge_max >= 0.0)))
        throw std::runtime_error("--sponge takes WIDTH > 0 and SIGMA_MAX >= 0");
      if (sponge && ((wave_steps <= 0 && n_harmonic <= 0) || n_members > 0))
        throw std::runtime_error("--sponge damps --wave STEPS DT [--direct] [--irk gauss|radau] or --harmonic K W0 W1, without --ensemble");
      LODParameters<2, 1> par;
      par.n_global_refinements  = argc > 1 ? std::atoi(argv[1]) : 3;
      par.n_subdivisions        = argc > 2 ? std::atoi(argv[2]) : 4;
      par.oversampling          = argc > 3 ? std::atoi(argv[3]) : 1;
      par.LOD_stabilization     = argc > 4 ? std::atoi(argv[4]) != 0 : true;
      par.constant_coefficients = false;
      par.n_members             = n_members > 0 ? (unsigned int)n_members : 1u;
      std::srand(1);
      for (int k = 0; k < member; ++k)
        problem_parameter<2>(1, 100, 3); // the draws of the members before this one
      Problem problem(par, 1, 100, 3);
      problem.run();
      problem.quiet_load(quiet_load);
      // the sources and their wavelet for the next loop of `steps` steps: sampled at t_k, with --irk at the stage times
      auto drive = [&](const int steps, const double dt, const bool ensemble) {
        if (sources.empty())
          return;
        problem.create_sources(sources, ensemble);
        std::vector<double> times;
        if (irk >= 0)
          {
            const double r3 = std::sqrt(3.0);
            const double c[2] = {irk == SLOD_IRK_GAUSS2 ? 0.5 - r3 / 6.0 : 1.0 / 3.0, irk == SLOD_IRK_GAUSS2 ? 0.5 + r3 / 6.0 : 1.0};
            for (int k = 0; k < steps; ++k)
              for (int i = 0; i < 2; ++i)
                times.push_back(((double)k + c[i]) * dt);
          }
        else
          for (int k = 0; k <= steps; ++k)
            times.push_back((double)k * dt);
        std::vector<double> signal;
        for (const double t : times)
          signal.insert(signal.end(), sources.size(), ricker(t, ricker_f0, ricker_t0, ricker_amp));
        problem.drive_next(signal, (unsigned int)times.size());
      };
      // the sponge layer sigma = SIGMA_MAX max(0, 1 - d / WIDTH)^2 per fine element, d the distance of its centre from the rim
      auto set_sponge = [&](Problem &pr) {
        const std::size_t   NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
        std::vector<double> sigma(NE * NE);
        for (std::size_t ey = 0; ey < NE; ++ey)
          for (std::size_t ex = 0; ex < NE; ++ex)
            {
              const double x = ((double)ex + 0.5) / (double)NE, y = ((double)ey + 0.5) / (double)NE;
              const double d = std::min(std::min(x, 1.0 - x), std::min(y, 1.0 - y));
              const double r = std::max(0.0, 1.0 - d / sponge_width);
              sigma[ey * NE + ex] = sponge_max * (r * r);
            }
        pr.assemble_damping_matrix(sigma);
        std::printf("sponge: width = %g, sigma_max = %.12e, zero coarse rows of D = %u\n", sponge_width, sponge_max,
                    pr.damping_zero_rows());
      };
      double s1 = 0, s2 = 0;
      for (const auto &p : problem.get_patches())
        for (std::size_t i = 0; i < p.basis_function[0].size(); ++i)
          {
            s1 += p.basis_function[0][i];
            s2 += p.basis_function_premultiplied[0][i] * p.basis_function[0][i];
          }
      std::printf("basis digest: sum phi = %.12e, sum phi.psi = %.12e\n", s1, s2);
      std::printf("basis build time: %.3f ms\n", problem.basis_build_seconds() * 1e3);
      if (argc > 5)
        problem.dump(argv[5]);
      if (compare)
        {
          problem.assemble_global_matrix();
          problem.assemble_and_solve_fem_problem();
          if (coarse)
            problem.assemble_and_solve_coarse_fem_problem();
          problem.solve();
          problem.compare_lod_with_fem();
          const slod_error_norms &e = problem.error_LOD_FEMh(), &u = problem.norms_FEMh();
          const double h1 = std::sqrt(e.l2[0] * e.l2[0] + e.h1_semi[0] * e.h1_semi[0]),
                       uh1 = std::sqrt(u.l2[0] * u.l2[0] + u.h1_semi[0] * u.h1_semi[0]);
          if (coarse)
            {
              const slod_error_norms &c = problem.error_FEMH_FEMh();
              const double ch1 = std::sqrt(c.l2[0] * c.l2[0] + c.h1_semi[0] * c.h1_semi[0]);
              std::printf("FEM(H) vs reference FEM(h)\n");
              std::printf("  L2     error = %.12e  (relative %.6e)\n", c.l2[0], c.l2[0] / u.l2[0]);
              std::printf("  H1     error = %.12e  (relative %.6e)\n", ch1, ch1 / uh1);
              std::printf("  Linfty error = %.12e  (relative %.6e)\n", c.linf[0], c.linf[0] / u.linf[0]);
              std::printf("  energy error = %.12e  (relative %.6e)\n", c.energy, c.energy / u.energy);
            }
          std::printf("SLOD vs reference FEM(h)\n");
          std::printf("  L2     error = %.12e  (relative %.6e)\n", e.l2[0], e.l2[0] / u.l2[0]);
          std::printf("  H1     error = %.12e  (relative %.6e)\n", h1, h1 / uh1);
          std::printf("  Linfty error = %.12e  (relative %.6e)\n", e.linf[0], e.linf[0] / u.linf[0]);
          std::printf("  energy error = %.12e  (relative %.6e)\n", e.energy, e.energy / u.energy);
        }
      if (n_loads > 0)
        {
          if (!compare)
            problem.assemble_global_matrix();
          std::vector<SineLoad> loads;
          for (int k = 1; k <= n_loads; ++k)
            loads.emplace_back(k);
          std::vector<const Function<2> *> ptrs;
          for (const auto &l : loads)
            ptrs.push_back(&l);
          problem.solve_multi(ptrs);
          if (compare)
            problem.compare_multi_with_fem();
          for (int k = 0; k < n_loads; ++k)
            {
              std::printf("load %d: iterations = %d, relative residual = %.6e\n", k + 1, problem.multi_iterations()[k],
                          problem.multi_rel_residuals()[k]);
              if (compare)
                std::printf("load %d: L2 error = %.12e, energy error = %.12e\n", k + 1,
                            problem.error_multi_LOD_FEMh()[k].l2[0], problem.error_multi_LOD_FEMh()[k].energy);
            }
        }
      if (heat_steps > 0)
        {
          if (!compare)
            {
              if (n_loads <= 0)
                problem.assemble_global_matrix();
              problem.assemble_and_solve_fem_problem();
              problem.solve();
            }
          problem.assemble_mass_matrix();
          const bool record = !receivers.empty() && n_members <= 0; // with --ensemble the ensemble loop records
          if (record)
            {
              problem.create_receivers(receivers);
              problem.record_next((unsigned int)record_every);
            }
          if (n_members <= 0)
            drive(heat_steps, heat_dt, false);
          if (irk >= 0)
            problem.solve_heat_irk(irk, (unsigned int)heat_steps, heat_dt);
          else
            problem.solve_heat((unsigned int)heat_steps, heat_dt, 1.0, direct);
          if (record)
            print_trace(problem, "heat", heat_dt, member);
          problem.compare_heat_with_lod();
          if (irk >= 0)
            print_irk_factor(irk_name, problem.last_factor_info(), problem.last_factor_inertia());
          else if (direct)
            print_factor(problem.last_factor_info());
          for (int k = 0; k < heat_steps; ++k)
            if (direct || irk >= 0)
              std::printf("heat step %d\n", k + 1);
            else
              std::printf("heat step %d: iterations = %d, relative residual = %.6e\n", k + 1, problem.heat_iterations()[k],
                          problem.heat_rel_residuals()[k]);
          const slod_error_norms &e = problem.error_heat_LOD(), &u = problem.norms_LOD();
          const double h1 = std::sqrt(e.l2[0] * e.l2[0] + e.h1_semi[0] * e.h1_semi[0]),
                       uh1 = std::sqrt(u.l2[0] * u.l2[0] + u.h1_semi[0] * u.h1_semi[0]);
          std::printf("SLOD heat flow at T = %g vs elliptic SLOD solution\n", heat_steps * heat_dt);
          std::printf("  L2     error = %.12e  (relative %.6e)\n", e.l2[0], e.l2[0] / u.l2[0]);
          std::printf("  H1     error = %.12e  (relative %.6e)\n", h1, h1 / uh1);
          std::printf("  Linfty error = %.12e  (relative %.6e)\n", e.linf[0], e.linf[0] / u.linf[0]);
          std::printf("  energy error = %.12e  (relative %.6e)\n", e.energy, e.energy / u.energy);
        }
      if (n_eigs > 0)
        {
          if (!compare && n_loads <= 0 && heat_steps <= 0)
            problem.assemble_global_matrix();
          if (heat_steps <= 0)
            problem.assemble_mass_matrix();
          if (direct && ldl)
            problem.solve_eigenproblem_near(shift, (unsigned int)n_eigs);
          else
            problem.solve_eigenproblem((unsigned int)n_eigs, direct, shift);
          for (int k = 0; k < n_eigs; ++k)
            std::printf("eigenvalue %d = %.12e, residual = %.3e\n", k + 1, problem.eigenvalues()[k], problem.eigen_residuals()[k]);
          if (direct)
            {
              std::printf("eigensolver: outer iterations = %d, direct\n", problem.eigen_outer_iterations());
              if (ldl)
                print_ldl_factor(problem.last_factor_info(), problem.last_factor_inertia());
              else
                print_factor(problem.last_factor_info());
            }
          else
            {
              std::printf("eigensolver: outer iterations = %d, inner iterations =", (int)problem.eigen_inner_iterations().size());
              for (const int it : problem.eigen_inner_iterations())
                std::printf(" %d", it);
              std::printf("\n");
            }
          for (int k = 0; k < n_eigs; ++k)
            std::printf("eigenfunction %d: L2 norm = %.12e\n", k + 1, problem.eigenfunction_norms()[k].l2[0]);
        }
      if (wave_steps > 0)
        {
          if (!compare && heat_steps <= 0)
            {
              if (n_loads <= 0 && n_eigs <= 0)
                problem.assemble_global_matrix();
              problem.assemble_and_solve_fem_problem();
            }
          if (heat_steps <= 0 && n_eigs <= 0)
            problem.assemble_mass_matrix();
          const bool record = !receivers.empty() && n_members <= 0; // with --ensemble the ensemble loop records
          if (record)
            {
              problem.create_receivers(receivers);
              problem.record_next((unsigned int)record_every);
            }
          if (n_members <= 0)
            drive(wave_steps, wave_dt, false);
          if (sponge)
            set_sponge(problem);
          if (irk >= 0)
            problem.solve_wave_irk(irk, (unsigned int)wave_steps, wave_dt);
          else
            problem.solve_wave((unsigned int)wave_steps, wave_dt, 0.25, 0.5, direct);
          if (record)
            print_trace(problem, "wave", wave_dt, member);
          if (irk >= 0)
            print_irk_factor(irk_name, problem.last_factor_info(), problem.last_factor_inertia());
          else if (direct)
            print_factor(problem.last_factor_info());
          for (int k = 0; k < wave_steps; ++k)
            if (direct || irk >= 0)
              std::printf("wave step %d: kinetic = %.12e, potential = %.12e, work = %.12e\n", k + 1, problem.wave_kinetic()[k + 1],
                          problem.wave_potential()[k + 1], problem.wave_work()[k + 1]);
            else
              std::printf("wave step %d: iterations = %d, relative residual = %.6e, kinetic = %.12e, potential = %.12e, work = %.12e\n",
                        k + 1, problem.wave_iterations()[k], problem.wave_rel_residuals()[k], problem.wave_kinetic()[k + 1],
                        problem.wave_potential()[k + 1], problem.wave_work()[k + 1]);
          std::printf("SLOD wave at T = %g: L2 norm = %.12e\n", wave_steps * wave_dt, problem.norms_wave().l2[0]);
        }
      if (n_harmonic > 0)
        {
          if (!compare && heat_steps <= 0 && wave_steps <= 0)
            {
              if (n_loads <= 0 && n_eigs <= 0)
                problem.assemble_global_matrix();
              problem.assemble_and_solve_fem_problem();
            }
          if (heat_steps <= 0 && n_eigs <= 0 && wave_steps <= 0)
            problem.assemble_mass_matrix();
          std::vector<double> omegas((std::size_t)n_harmonic);
          for (int k = 0; k < n_harmonic; ++k)
            omegas[k] = n_harmonic > 1 ? harmonic_w0 + k * ((harmonic_w1 - harmonic_w0) / (n_harmonic - 1)) : harmonic_w0;
          if (sponge && wave_steps <= 0)
            set_sponge(problem);
          problem.solve_harmonic(omegas, damp_mass, damp_stiff);
          for (int k = 0; k < n_harmonic; ++k)
            std::printf("harmonic %d: omega = %.12e, growth = %.6e, relative residual = %.6e, amplitude = %.12e, power = %.12e\n",
                        k + 1, omegas[k], problem.harmonic_growth()[k], problem.harmonic_residuals()[k],
                        problem.harmonic_amplitude()[k], problem.harmonic_power()[k]);
        }
      if (n_members > 0)
        {
          problem.solve_ensemble();
          for (int k = 0; k < n_members; ++k)
            std::printf("member %d: iterations = %d, relative residual = %.6e\n", k, problem.ensemble_iterations()[k],
                        problem.ensemble_rel_residuals()[k]);
          std::printf("SLOD ensemble of %d: L2 norm of the mean = %.12e, of the standard deviation = %.12e\n", n_members,
                      problem.norms_ensemble_mean().l2[0], problem.norms_ensemble_deviation().l2[0]);
          if (precond_member >= 0)
            {
              problem.solve_ensemble_precond((unsigned int)precond_member);
              for (int k = 0; k < n_members; ++k)
                std::printf("member %d: PCG iterations = %d, Jacobi-CG iterations = %d\n", k, problem.ensemble_precond_iterations()[k],
                            problem.ensemble_precond_jacobi_iterations()[k]);
            }
          const bool irk_ensemble = irk >= 0 && (heat_steps > 0 || wave_steps > 0);
          if (((heat_steps > 0 || wave_steps > 0 || n_eigs > 0) && direct) || n_harmonic > 0 || irk_ensemble)
            problem.assemble_mass_matrix_ensemble();
          if (n_harmonic > 0)
            {
              std::vector<double> omegas((std::size_t)n_harmonic);
              for (int k = 0; k < n_harmonic; ++k)
                omegas[k] = n_harmonic > 1 ? harmonic_w0 + k * ((harmonic_w1 - harmonic_w0) / (n_harmonic - 1)) : harmonic_w0;
              problem.solve_harmonic_ensemble(omegas, damp_mass, damp_stiff);
              for (int k = 0; k < n_harmonic; ++k)
                {
                  std::vector<double> amplitude;
                  for (int m = 0; m < n_members; ++m)
                    {
                      const std::size_t at = (std::size_t)k * n_members + m;
                      std::printf("harmonic %d member %d: omega = %.12e, growth = %.6e, relative residual = %.6e, amplitude = %.12e, "
                                  "power = %.12e\n",
                                  k + 1, m, omegas[k], problem.harmonic_ensemble_growth()[at], problem.harmonic_ensemble_residuals()[at],
                                  problem.harmonic_ensemble_amplitude()[at], problem.harmonic_ensemble_power()[at]);
                      amplitude.push_back(problem.harmonic_ensemble_amplitude()[at]);
                    }
                  double mean, dev;
                  mean_and_deviation(amplitude, mean, dev);
                  std::printf("harmonic %d amplitude over the ensemble of %d: mean = %.12e, standard deviation = %.12e\n", k + 1,
                              n_members, mean, dev);
                }
              std::printf("SLOD harmonic ensemble of %d at omega = %.12e: L2 norm of the mean = %.12e (real), %.12e (imaginary), of the "
                          "standard deviation = %.12e (real), %.12e (imaginary)\n",
                          n_members, omegas[problem.harmonic_ensemble_peak()], problem.norms_harmonic_ensemble_real_mean().l2[0],
                          problem.norms_harmonic_ensemble_imag_mean().l2[0], problem.norms_harmonic_ensemble_real_deviation().l2[0],
                          problem.norms_harmonic_ensemble_imag_deviation().l2[0]);
            }
          if (heat_steps > 0 && direct)
            {
              if (!receivers.empty())
                {
                  problem.create_receivers(receivers, true);
                  problem.record_next((unsigned int)record_every);
                }
              drive(heat_steps, heat_dt, true);
              problem.solve_heat_ensemble((unsigned int)heat_steps, heat_dt, 1.0);
              if (!receivers.empty())
                print_trace(problem, "heat", heat_dt, 0);
              print_factor(problem.last_factor_info());
              for (int j = 0; j < heat_steps; ++j)
                for (int k = 0; k < n_members; ++k)
                  {
                    const slod_error_norms &e = problem.error_heat_ensemble()[(std::size_t)j * n_members + k];
                    std::printf("member %d heat step %d: L2 distance = %.12e, energy distance = %.12e\n", k, j + 1, e.l2[0], e.energy);
                  }
              std::printf("SLOD heat ensemble of %d at T = %g: L2 norm of the mean = %.12e, of the standard deviation = %.12e\n",
                          n_members, heat_steps * heat_dt, problem.norms_heat_ensemble_mean().l2[0],
                          problem.norms_heat_ensemble_deviation().l2[0]);
            }
          if (wave_steps > 0 && direct)
            {
              if (!receivers.empty())
                {
                  problem.create_receivers(receivers, true);
                  problem.record_next((unsigned int)record_every);
                }
              drive(wave_steps, wave_dt, true);
              problem.solve_wave_ensemble((unsigned int)wave_steps, wave_dt, 0.25, 0.5);
              if (!receivers.empty())
                print_trace(problem, "wave", wave_dt, 0);
              print_factor(problem.last_factor_info());
              for (int k = 0; k < n_members; ++k)
                for (int j = 1; j <= wave_steps; ++j)
                  {
                    const std::size_t at = (std::size_t)j * n_members + k;
                    std::printf("member %d wave step %d: kinetic = %.12e, potential = %.12e, work = %.12e\n", k, j,
                                problem.wave_ensemble_kinetic()[at], problem.wave_ensemble_potential()[at],
                                problem.wave_ensemble_work()[at]);
                  }
              std::printf("SLOD wave ensemble of %d at T = %g: L2 norm of the mean = %.12e, of the standard deviation = %.12e\n",
                          n_members, wave_steps * wave_dt, problem.norms_wave_ensemble_mean().l2[0],
                          problem.norms_wave_ensemble_deviation().l2[0]);
            }
          if (heat_steps > 0 && irk >= 0)
            {
              if (!receivers.empty())
                {
                  problem.create_receivers(receivers, true);
                  problem.record_next((unsigned int)record_every);
                }
              drive(heat_steps, heat_dt, true);
              problem.solve_heat_irk_ensemble(irk, (unsigned int)heat_steps, heat_dt);
              if (!receivers.empty())
                print_trace(problem, "heat", heat_dt, 0);
              print_irk_factor(irk_name, problem.last_factor_info(), problem.last_factor_inertia());
              for (int j = 0; j < heat_steps; ++j)
                for (int k = 0; k < n_members; ++k)
                  {
                    const slod_error_norms &e = problem.error_heat_ensemble()[(std::size_t)j * n_members + k];
                    std::printf("member %d irk heat step %d: L2 distance = %.12e, energy distance = %.12e\n", k, j + 1, e.l2[0], e.energy);
                  }
              std::printf("SLOD irk heat ensemble of %d at T = %g: L2 norm of the mean = %.12e, of the standard deviation = %.12e\n",
                          n_members, heat_steps * heat_dt, problem.norms_heat_ensemble_mean().l2[0],
                          problem.norms_heat_ensemble_deviation().l2[0]);
            }
          if (wave_steps > 0 && irk >= 0)
            {
              if (!receivers.empty())
                {
                  problem.create_receivers(receivers, true);
                  problem.record_next((unsigned int)record_every);
                }
              drive(wave_steps, wave_dt, true);
              problem.solve_wave_irk_ensemble(irk, (unsigned int)wave_steps, wave_dt);
              if (!receivers.empty())
                print_trace(problem, "wave", wave_dt, 0);
              print_irk_factor(irk_name, problem.last_factor_info(), problem.last_factor_inertia());
              for (int k = 0; k < n_members; ++k)
                for (int j = 1; j <= wave_steps; ++j)
                  {
                    const std::size_t at = (std::size_t)j * n_members + k;
                    std::printf("member %d irk wave step %d: kinetic = %.12e, potential = %.12e, work = %.12e\n", k, j,
                                problem.wave_ensemble_kinetic()[at], problem.wave_ensemble_potential()[at],
                                problem.wave_ensemble_work()[at]);
                  }
              std::printf("SLOD irk wave ensemble of %d at T = %g: L2 norm of the mean = %.12e, of the standard deviation = %.12e\n",
                          n_members, wave_steps * wave_dt, problem.norms_wave_ensemble_mean().l2[0],
                          problem.norms_wave_ensemble_deviation().l2[0]);
            }
        }
      if (n_members > 0 && n_eigs > 0 && direct)
        {
          if (ldl)
            problem.solve_eigenproblem_ensemble_near(shift, (unsigned int)n_eigs);
          else
            problem.solve_eigenproblem_ensemble((unsigned int)n_eigs, shift);
          if (ldl)
            print_ldl_factor(problem.last_factor_info(), problem.factor_inertia_ensemble()[0]);
          else
            print_factor(problem.last_factor_info());
          const int m = problem.eigen_ensemble_block();
          for (int k = 0; k < n_members; ++k)
            {
              if (ldl)
                std::printf("member %d factor: n_negative = %d, growth = %.6e\n", k, problem.factor_inertia_ensemble()[k].n_negative,
                            problem.factor_inertia_ensemble()[k].norm_factor / problem.factor_inertia_ensemble()[k].norm_matrix);
              for (int j = 0; j < n_eigs; ++j)
                std::printf("member %d eigenvalue %d = %.12e, residual = %.3e\n", k, j + 1,
                            problem.eigenvalues_ensemble()[(std::size_t)k * m + j], problem.eigen_residuals_ensemble()[(std::size_t)k * m + j]);
              std::printf("member %d eigensolver: outer iterations = %d, direct\n", k, problem.eigen_outer_iterations_ensemble()[k]);
            }
          if (ldl)
            {
              std::vector<double> below;
              for (int k = 0; k < n_members; ++k)
                below.push_back((double)problem.factor_inertia_ensemble()[k].n_negative);
              double mean, dev;
              mean_and_deviation(below, mean, dev);
              std::printf("n_negative over the ensemble of %d: mean = %.12e, standard deviation = %.12e\n", n_members, mean, dev);
            }
          for (int j = 0; j < n_eigs; ++j)
            {
              // sample mean and unbiased standard deviation over the members, summed in ascending member order
              double mean = 0.0, var = 0.0;
              for (int k = 0; k < n_members; ++k)
                mean += problem.eigenvalues_ensemble()[(std::size_t)k * m + j];
              mean /= n_members;
              for (int k = 0; k < n_members; ++k)
                {
                  const double d = problem.eigenvalues_ensemble()[(std::size_t)k * m + j] - mean;
                  var += d * d;
                }
              var = n_members > 1 ? var / (n_members - 1) : 0.0;
              std::printf("eigenvalue %d over the ensemble of %d: mean = %.12e, standard deviation = %.12e\n", j + 1, n_members, mean,
                          std::sqrt(var));
            }
        }
      if (n_perturb > 0)
        {
          if (!compare && n_loads <= 0 && heat_steps <= 0 && n_eigs <= 0 && wave_steps <= 0 && n_harmonic <= 0)
            problem.assemble_global_matrix();
          if (!compare && heat_steps <= 0 && wave_steps <= 0 && n_harmonic <= 0)
            problem.assemble_and_solve_fem_problem(); // the load C^T f of solve(); f = 1 does not see the coefficient
          if (reuse_factor)
            problem.factor_for_reuse();
          problem.flip_coefficient_cells((unsigned int)n_perturb);
          const unsigned int n_dirty = problem.refresh_after_coefficient_change();
          problem.solve();
          if (reuse_factor)
            problem.solve_precond();
          const std::vector<double> a_refresh = problem.lod_matrix_values(), u_refresh = problem.lod_solution();
          std::printf("perturbation of %d coefficient cells: dirty patches = %u of %u\n", n_perturb, n_dirty,
                      (unsigned int)problem.get_patches().size());
          std::printf("rebuild from scratch:\n");
          std::srand(1); // the draws of the first problem, then the same flips
          Problem rebuilt(par, 1, 100, 3);
          rebuilt.flip_coefficient_cells((unsigned int)n_perturb);
          rebuilt.run();
          rebuilt.assemble_global_matrix();
          rebuilt.assemble_and_solve_fem_problem();
          rebuilt.solve();
          const std::vector<double> a_rebuild = rebuilt.lod_matrix_values(), u_rebuild = rebuilt.lod_solution();
          const auto max_diff = [](const std::vector<double> &a, const std::vector<double> &b, double &scale) {
            double d = 0.0;
            scale    = 0.0;
            for (std::size_t i = 0; i < a.size(); ++i)
              {
                d     = std::max(d, std::fabs(a[i] - b[i]));
                scale = std::max(scale, std::fabs(b[i]));
              }
            return d;
          };
          double       a_scale = 0.0, u_scale = 0.0;
          const double a_diff = max_diff(a_refresh, a_rebuild, a_scale), u_diff = max_diff(u_refresh, u_rebuild, u_scale);
          std::printf("  max |A_refresh - A_rebuild| = %.6e  (max |A_rebuild| = %.6e)\n", a_diff, a_scale);
          std::printf("  max |u_refresh - u_rebuild| = %.6e  (max |u_rebuild| = %.6e)\n", u_diff, u_scale);
          if (reuse_factor)
            {
              const double p_diff = max_diff(problem.precond_solution(), u_rebuild, u_scale);
              std::printf("stale factor as preconditioner: dirty patches = %u of %u, PCG iterations = %d, Jacobi-CG iterations = %d\n",
                          n_dirty, (unsigned int)problem.get_patches().size(), problem.precond_iterations(),
                          problem.precond_jacobi_iterations());
              std::printf("  max |u_pcg - u_rebuild| = %.6e  (max |u_rebuild| = %.6e)\n", p_diff, u_scale);
            }
        }
    }
  catch (std::exception &exc)
    {
      std::cerr << std::endl
                << "----------------------------------------------------" << std::endl
                << "Exception on processing: " << std::endl
                << exc.what() << std::endl
                << "Aborting!" << std::endl
                << "----------------------------------------------------" << std::endl;
      return 1; // as app/main_Diffusion.cc:23-47
    }
  return 0;
}
