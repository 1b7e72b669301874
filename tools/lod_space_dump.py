#!/usr/bin/env python3
"""Dump every bit-reproducible output of the LOD-space entry points into one .npz, so that two builds of the library
can be compared word for word:

  python tools/lod_space_dump.py out.npz                  run the library of this tree
  python tools/lod_space_dump.py --compare a.npz b.npz    one line per array, exit status 1 on any difference

Configurations: the four of the mass-matrix tests (16-25 patches) and nref 3, n_sub 4, l = 1 (64 patches), D100
coefficient; n_rhs = 1, 3, 65 (3 puts several rows into one wave, 65 crosses the 64-column chunk).  Per configuration:
values and cols of slod_lod_matrix and of slod_lod_mass_matrix (rho = 1 and a seeded random rho), the symmetrised
stiffness and slod_lod_eigs (n_eig 4, default guard columns, the library's start block, max_outer 20); per n_rhs:
lod_rhs_multi, lod_apply, lod_inner, lod_solve_multi, three lod_theta_steps (theta 1 and 1/2, distinct loads),
lod_newmark_accel, three lod_newmark_steps (beta 1/4 undamped, beta 0 damped) with both energies, and
lod_reconstruct_multi.  slod_lod_solve (scalar, atomic sums) is not bit-reproducible and is left out.

The calls on banded factors, on the four small configurations (DIRECT): the pivot ranges of the Cholesky factors of M
and of the step matrices (lod_matrix_combine of the symmetrised stiffness and M), lod_eigs_direct on the LDL^T factor of
the stiffness and lod_eigs_shift_direct on that of A - sigma M, sigma between the second and third eigenvalue of
lod_eigs; per n_rhs a factor solve, lod_theta_steps_direct, lod_newmark_accel_direct and lod_newmark_steps_direct with
the parameters of the CG calls above.  Under <name>/ens/: K = 3 members of one handle with seeded D100 coefficients of
their own, lod_inner_ensemble, lod_theta_steps_ensemble_direct, both Newmark ensemble calls and
lod_eigs_ensemble_direct, a column per member.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-slod_amd"))

SEED = 20250614
CONFIGS = {"s1": dict(nref=2, n_sub=2, oversampling=1, spacedim=1),
           "clipped": dict(nref=2, n_sub=4, oversampling=2, spacedim=1),
           "s2": dict(nref=2, n_sub=2, oversampling=1, spacedim=2),
           "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1),
           "c1": dict(nref=3, n_sub=4, oversampling=1, spacedim=1)}
DIRECT = ("s1", "clipped", "s2", "rowmajor")      # the configurations that also run the calls on factors
N_RHS = (1, 3, 65)
K_ENS = 3
THETAS = ((1.0, 0.01), (0.5, 0.01))               # (theta, dt)
# tag, beta, dt, damp_mass, damp_stiff (gamma = 1/2): the damped run has the mass product in its right-hand side
NEWMARK = (("newmark_quarter_", 0.25, 0.05, 0.0, 0.0), ("newmark_central_", 0.0, 1e-4, 0.5, 1e-4))
STEPS, TOL, MAXIT = 3, 1e-12, 5000


def dump(path):
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_space_dump.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    out = {}

    def f64(*shape):
        return torch.zeros(*shape, dtype=torch.float64, device=dev)

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().copy()

    def step_matrices(nmat, combine, factor, A, M):
        """The Cholesky factors of M, of M + theta dt A and of the Newmark step matrices, by tag; combine(alpha, a, beta, b,
        out) and factor(values) are those of one matrix or of an ensemble."""
        fac = {"mass": factor(M)}
        coef = [("theta%g" % theta, 1.0, theta * dt) for theta, dt in THETAS]
        coef += [(tag, 1.0 + 0.5 * dt * dm, beta * dt * dt + 0.5 * dt * ds) for tag, beta, dt, dm, ds in NEWMARK]
        for tag, alpha, beta in coef:
            S = f64(*nmat)
            combine(alpha, M.data_ptr(), beta, A.data_ptr(), S.data_ptr())
            fac[tag] = factor(S)
        return fac

    def pivots(key, fac):
        for tag, f in fac.items():
            out[key + "factor_pivots_" + tag.rstrip("_")] = np.array([f.info.min_pivot, f.info.max_pivot])

    def ensemble(kw, key):
        """K_ENS members of one handle, a column per member: the calls on an ensemble matrix and an ensemble factor."""
        K, s = K_ENS, kw["spacedim"]
        g = slod_amd.Slod(stabilize=1, n_problems=K, **kw)
        for k in range(K):
            for f in range(s):
                g.set_coefficient(f, fill_coefficient(SEED + 100 * (k + 1) + f, "D100", g.NE), problem=k)
        NP, cap = g.num_patches, g.lod_row_capacity()
        plan = g.plan(np.arange(K * NP, dtype=np.uint32))
        b, q = f64(K * NP * plan.stride), f64(K * NP * plan.stride)
        plan.execute(b.data_ptr(), q.data_ptr())
        plan.status()
        nrow, nmat = NP * s, NP * cap * s * s
        rng = np.random.default_rng(12)
        raw, A, M = f64(nmat, K), f64(nmat, K), f64(nmat, K)
        cols, mcols = (torch.zeros(NP * cap, dtype=torch.int32, device=dev) for _ in range(2))
        g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), plan.stride, K, raw.data_ptr(), cols.data_ptr())
        g.lod_mass_matrix_ensemble(b.data_ptr(), plan.stride, K, M.data_ptr(), mcols.data_ptr())
        g.lod_matrix_symmetrize_ensemble(raw.data_ptr(), cols.data_ptr(), K, A.data_ptr())
        out[key + "matrix_values"], out[key + "mass_values"] = host(A), host(M)
        ptr = (A.data_ptr(), M.data_ptr(), cols.data_ptr())
        fac = step_matrices((nmat, K), lambda al, a, be, b_, o: g.lod_matrix_combine_ensemble(al, a, be, b_, K, o),
                            lambda v: g.lod_factor_ensemble(v.data_ptr(), cols.data_ptr(), K), A, M)
        pivots(key, fac)
        L = torch.from_numpy(rng.uniform(-1.0, 1.0, (STEPS + 1, nrow, K))).to(dev)
        Xr = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, K))).to(dev)
        Y = f64(nrow, K)
        g.lod_apply_ensemble(A.data_ptr(), cols.data_ptr(), Xr.data_ptr(), Y.data_ptr(), K)
        out[key + "inner"] = g.lod_inner_ensemble(A.data_ptr(), cols.data_ptr(), Xr.data_ptr(), Y.data_ptr(), K).copy()
        for theta, dt in THETAS:
            u = Xr.clone() * 1e-3
            g.lod_theta_steps_ensemble_direct(fac["theta%g" % theta], A.data_ptr(), cols.data_ptr(), dt, theta, STEPS, K,
                                              u.data_ptr(), d_load=L.data_ptr(), load_step_stride=nrow * K)
            out[key + "theta%g_u" % theta] = host(u)
        for tag, beta, dt, dm, ds in NEWMARK:
            u, v, a = Xr.clone() * 1e-3, Y.clone() * 1e-3, f64(nrow, K)
            g.lod_newmark_accel_ensemble_direct(fac["mass"], *ptr, K, u.data_ptr(), v.data_ptr(), a.data_ptr(),
                                                d_load=L[0].data_ptr(), damp_mass=dm, damp_stiff=ds)
            out[key + tag + "accel"] = host(a)
            kin, pot = g.lod_newmark_steps_ensemble_direct(fac[tag], *ptr, dt, STEPS, K, u.data_ptr(), v.data_ptr(), a.data_ptr(),
                                                           beta=beta, d_load=L.data_ptr(), load_step_stride=nrow * K,
                                                           damp_mass=dm, damp_stiff=ds)
            for nm, arr in (("u", host(u)), ("v", host(v)), ("a", host(a)), ("kinetic", kin), ("potential", pot)):
                out[key + tag + nm] = arr
        m = min(64, nrow, 8)
        X = f64(nrow, K * m)
        f = g.lod_factor_ldl_ensemble(A.data_ptr(), cols.data_ptr(), K)
        el, er, status, rc = g.lod_eigs_ensemble_direct(f, *ptr, K, 4, X.data_ptr(), max_outer=20)
        for nm, arr in (("lambda", el), ("residual", er), ("status", status), ("X", host(X))):
            out[key + "eigs_" + nm] = arr
        g.close()

    for name, kw in CONFIGS.items():
        g = slod_amd.Slod(stabilize=1, **kw)
        s, NP, cap, NE = kw["spacedim"], g.num_patches, g.lod_row_capacity(), g.NE
        for f in range(s):
            g.set_coefficient(f, fill_coefficient(SEED + f, "D100", NE))
        ids = np.arange(NP, dtype=np.uint32)
        plan = g.plan(ids)
        b, q = f64(NP * plan.stride), f64(NP * plan.stride)
        plan.execute(b.data_ptr(), q.data_ptr())
        plan.status()
        nrow, nfine, nmat = NP * s, (NE + 1) ** 2 * s, NP * cap * s * s
        rng = np.random.default_rng(11)
        A, cols = f64(nmat), torch.zeros(NP * cap, dtype=torch.int32, device=dev)
        g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, A.data_ptr(), cols.data_ptr())
        out[name + "/matrix_values"], out[name + "/matrix_cols"] = host(A), host(cols)
        M = f64(nmat)
        for tag, rho in (("rho_random", torch.from_numpy(rng.uniform(0.5, 2.0, NE * NE)).to(dev)), ("rho_one", None)):
            mcols = torch.zeros_like(cols)
            g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, M.data_ptr(), mcols.data_ptr(),
                              d_rho=None if rho is None else rho.data_ptr())
            out[name + "/mass_values_" + tag], out[name + "/mass_cols_" + tag] = host(M), host(mcols)
        sym = f64(nmat)                                  # M holds the rho = 1 mass from here on
        g.lod_matrix_symmetrize(A.data_ptr(), cols.data_ptr(), sym.data_ptr())
        out[name + "/symmetrize"] = host(sym)
        ptr = (sym.data_ptr(), M.data_ptr(), cols.data_ptr())

        X = f64(nrow, min(64, nrow, 8))                  # n_eig = 4 and the binding's default guard columns
        lam, res, its = g.lod_eigs(*ptr, 4, X.data_ptr(), max_outer=20)
        out[name + "/eigs_lambda"], out[name + "/eigs_residual"], out[name + "/eigs_inner"] = lam, res, its
        out[name + "/eigs_X"] = host(X)

        direct = name in DIRECT
        if direct:
            fac = step_matrices((nmat,), g.lod_matrix_combine, lambda v: g.lod_factor(v.data_ptr(), cols.data_ptr()), sym, M)
            pivots(name + "/", fac)
            sigma = 0.5 * (lam[1] + lam[2])
            shifted = f64(nmat)
            g.lod_matrix_combine(1.0, sym.data_ptr(), -sigma, M.data_ptr(), shifted.data_ptr())
            for tag, f, sigma in (("eigs_direct_", g.lod_factor_ldl(sym.data_ptr(), cols.data_ptr()), None),
                                  ("eigs_shift_direct_", g.lod_factor_ldl(shifted.data_ptr(), cols.data_ptr()), sigma)):
                X.zero_()
                if sigma is None:
                    el, er, rc = g.lod_eigs_direct(f, *ptr, 4, X.data_ptr(), max_outer=20)
                else:
                    el, er, rc = g.lod_eigs_shift_direct(f, sigma, *ptr, 4, X.data_ptr(), max_outer=20)
                for nm, arr in (("lambda", el), ("residual", er), ("outer", np.array([rc])), ("X", host(X))):
                    out[name + "/" + tag + nm] = arr
                f.close()
            ensemble(kw, name + "/ens/")

        for n in N_RHS:
            key = "%s/n%d/" % (name, n)
            # fine loads [level][column][fine], seeded; coarse loads [level][row][column]
            F = torch.from_numpy(rng.uniform(-1.0, 1.0, (STEPS + 1, n, nfine))).to(dev)
            L = f64(STEPS + 1, nrow, n)
            for k in range(STEPS + 1):
                g.lod_rhs_multi(ids, b.data_ptr(), plan.stride, F[k].data_ptr(), nfine, n, L[k].data_ptr(), n)
            out[key + "rhs_multi"] = host(L)
            Xr = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
            Y = f64(nrow, n)
            g.lod_apply(A.data_ptr(), cols.data_ptr(), Xr.data_ptr(), Y.data_ptr(), n_rhs=n)
            out[key + "apply"] = host(Y)
            out[key + "inner"] = g.lod_inner(sym.data_ptr(), cols.data_ptr(), Xr.data_ptr(), Y.data_ptr(), n_rhs=n).copy()
            U = f64(nrow, n)
            its, res = g.lod_solve_multi(A.data_ptr(), cols.data_ptr(), L[0].data_ptr(), n, n, U.data_ptr(), n, TOL, MAXIT)
            out[key + "solve_u"], out[key + "solve_its"], out[key + "solve_res"] = host(U), its.copy(), res.copy()
            fine = f64(n, nfine)
            g.lod_reconstruct_multi(b.data_ptr(), plan.stride, U.data_ptr(), n, n, fine.data_ptr(), nfine)
            out[key + "reconstruct_multi"] = host(fine)
            for theta, dt in THETAS:
                u = Xr.clone() * 1e-3
                its, res = g.lod_theta_steps(*ptr, dt, theta, STEPS, u.data_ptr(), n_rhs=n, d_load=L.data_ptr(),
                                             load_step_stride=nrow * n, rel_tol=TOL, max_iterations=MAXIT)
                tag = key + "theta%g_" % theta
                out[tag + "u"], out[tag + "its"], out[tag + "res"] = host(u), its.copy(), res.copy()
            for tag, beta, dt, dm, ds in NEWMARK:
                u, v, a = Xr.clone() * 1e-3, Y.clone() * 1e-3, f64(nrow, n)
                its, res = g.lod_newmark_accel(*ptr, u.data_ptr(), v.data_ptr(), a.data_ptr(), n_rhs=n, d_load=L[0].data_ptr(),
                                               damp_mass=dm, damp_stiff=ds, rel_tol=TOL, max_iterations=MAXIT)
                out[key + tag + "accel"], out[key + tag + "accel_its"], out[key + tag + "accel_res"] = host(a), its.copy(), res.copy()
                its, res, kin, pot = g.lod_newmark_steps(*ptr, dt, STEPS, u.data_ptr(), v.data_ptr(), a.data_ptr(), beta=beta, n_rhs=n,
                                                         d_load=L.data_ptr(), load_step_stride=nrow * n, damp_mass=dm, damp_stiff=ds,
                                                         rel_tol=TOL, max_iterations=MAXIT)
                for nm, arr in (("u", host(u)), ("v", host(v)), ("a", host(a)), ("its", its.copy()), ("res", res.copy()),
                                ("kinetic", kin), ("potential", pot)):
                    out[key + tag + nm] = arr
            if not direct:
                continue
            key += "direct_"
            fac["mass"].solve(L[0].data_ptr(), U.data_ptr(), n_rhs=n)
            out[key + "factor_solve"] = host(U)
            for theta, dt in THETAS:
                u = Xr.clone() * 1e-3
                g.lod_theta_steps_direct(fac["theta%g" % theta], sym.data_ptr(), cols.data_ptr(), dt, theta, STEPS, u.data_ptr(),
                                         n_rhs=n, d_load=L.data_ptr(), load_step_stride=nrow * n)
                out[key + "theta%g_u" % theta] = host(u)
            for tag, beta, dt, dm, ds in NEWMARK:
                u, v, a = Xr.clone() * 1e-3, Y.clone() * 1e-3, f64(nrow, n)
                g.lod_newmark_accel_direct(fac["mass"], *ptr, u.data_ptr(), v.data_ptr(), a.data_ptr(), n_rhs=n,
                                           d_load=L[0].data_ptr(), damp_mass=dm, damp_stiff=ds)
                out[key + tag + "accel"] = host(a)
                kin, pot = g.lod_newmark_steps_direct(fac[tag], *ptr, dt, STEPS, u.data_ptr(), v.data_ptr(), a.data_ptr(), beta=beta,
                                                      n_rhs=n, d_load=L.data_ptr(), load_step_stride=nrow * n, damp_mass=dm,
                                                      damp_stiff=ds)
                for nm, arr in (("u", host(u)), ("v", host(v)), ("a", host(a)), ("kinetic", kin), ("potential", pot)):
                    out[key + tag + nm] = arr
    np.savez(path, **out)
    print("%d arrays -> %s" % (len(out), path))


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


def compare(pa, pb):
    za, zb = np.load(pa), np.load(pb)
    bad = sorted(set(za.files) ^ set(zb.files))
    for k in bad:
        print("%-48s only in one file" % k)
    for k in sorted(set(za.files) & set(zb.files)):
        a, b = za[k], zb[k]
        same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(words(a), words(b))
        print("%-48s %-8s %-14s %s" % (k, a.dtype, a.shape, "equal" if same else "DIFFERENT"))
        if not same:
            bad.append(k)
    print("%d arrays compared, %d differ" % (len(za.files), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    dump(sys.argv[1])
