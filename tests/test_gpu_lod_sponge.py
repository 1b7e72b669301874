"""GPU tests of the sponge layer: a third damping matrix D = C^T M_sigma C (slod_lod_mass_matrix with d_rho = sigma) in the
Newmark calls (slod_lod_newmark_*_damped), the three-term complex factor (slod_lod_factor_create_zldl3), the IRK wave
stepper (slod_lod_irk_wave_steps_damped_direct) and the frequency response (slod_lod_harmonic_response_damped), against the
dense yardsticks of lod_sponge_cases.py (checked on the CPU by test_lod_sponge_reference.py) and against themselves as
64-bit words.

Cases: the four of lod_ldl_cases.ldl_case (dense 16 rows, rowmajor 25, s2 128, morton16 256) with the sponge of the rule
(width 0.25, sigma_max = 4 sqrt(lam_1)); D is asserted bit-symmetric and semi-definite where it is built.  Bars: FORWARD =
1e-8 of max |reference| against a dense reference; the growth cap 1e4 is a condition on the yardstick before the library
is called; the backward error of the factor is that of test_gpu_lod_harmonic.py.
"""
import ctypes as C
import re

import numpy as np
import pytest

import lod_sponge_cases as sc
from lod_cases import NAN, _bits, _torch

pytestmark = pytest.mark.gpu

STEPS = 3
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _padded(a, ld):
    t = _nan(a.shape[0], ld)
    t[:, :a.shape[1]] = _dev(a)
    return t


def _sync():
    _torch()[0].cuda.synchronize()


def _np(t, n):
    return t.cpu().numpy()[:, :n]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _mats(c):
    return c.sym.data_ptr(), c.mvalues.data_ptr(), c.dvalues.data_ptr(), c.cols.data_ptr()


def _loads(loads, n, ld):
    """(tensor kept alive, d_load, ld_load, stride) for None, a constant [rows][>= n] or [levels][rows][>= n]."""
    if loads is None:
        return None, None, None, 0
    if loads.ndim == 2:
        t = _padded(loads[:, :n], ld)
        return t, t.data_ptr(), ld, 0
    t = _nan(loads.shape[0], loads.shape[1], ld)
    t[:, :, :n] = _dev(loads[:, :, :n])
    return t, t.data_ptr(), ld, loads.shape[1] * ld


def _step_matrix(c, dt, beta, gamma, dm, ds):
    """S of the damped Newmark step as the CG call builds it: two slod_lod_matrix_combine roundings."""
    S = _nan(c.sym.numel()).view(-1)
    c.g.lod_matrix_combine(1.0 + gamma * dt * dm, c.mvalues.data_ptr(), beta * dt * dt + gamma * dt * ds, c.sym.data_ptr(), S.data_ptr())
    c.g.lod_matrix_combine(1.0, S.data_ptr(), gamma * dt, c.dvalues.data_ptr(), S.data_ptr())
    _sync()
    return S


def _nm_factor(c, dt, beta, gamma, dm, ds, ldl=False):
    S = _step_matrix(c, dt, beta, gamma, dm, ds)
    return (c.g.lod_factor_ldl if ldl else c.g.lod_factor)(S.data_ptr(), c.cols.data_ptr())


def _nm_run(c, f, dt, beta, n_steps, state, loads, dm, ds, n, ld=None, first=0, damping=True, energies=True):
    """n_steps of the damped Newmark loop on (U, V, A) in place: on the factor f, or by CG with f None."""
    sym, mass, dmat, cols = _mats(c)
    ld = n if ld is None else ld
    U, V, A = state
    keep, d_load, ld_load, stride = _loads(loads, n, ld)
    if d_load is not None and stride:
        d_load += 8 * first * stride
    kw = dict(beta=beta, gamma=0.5, n_rhs=n, ld_u=ld, ld_v=ld, ld_a=ld, d_load=d_load, ld_load=ld_load, load_step_stride=stride,
              damp_mass=dm, damp_stiff=ds, energies=energies, d_damping=dmat if damping else None)
    if f is None:
        out = c.g.lod_newmark_steps(sym, mass, cols, dt, n_steps, U.data_ptr(), V.data_ptr(), A.data_ptr(), rel_tol=1e-13,
                                    max_iterations=5000, **kw)[2:]
    else:
        out = c.g.lod_newmark_steps_direct(f, sym, mass, cols, dt, n_steps, U.data_ptr(), V.data_ptr(), A.data_ptr(), **kw)
    _sync()
    return out


def _zfactor3(c, alpha, beta, gamma):
    sym, mass, dmat, cols = _mats(c)
    return c.g.lod_factor_zldl3(sym, mass, dmat, cols, alpha, beta, gamma)


def _irk_factor(c, scheme, dts, dm, ds):
    pairs = [c.g.lod_irk_coefficients(scheme, 2, dt, dm, ds) for dt in np.atleast_1d(dts)]
    return _zfactor3(c, [p[0] for p in pairs], [p[1] for p in pairs],
                     [c.g.lod_irk_damping_coefficient(scheme, dt) for dt in np.atleast_1d(dts)])


def _irk_run(c, f, scheme, dt, n_steps, u0, v0, dm, ds, loads=None, ld=None, member=0, damping=True, energies=True, first=0):
    sym, mass, dmat, cols = _mats(c)
    n = u0.shape[1]
    ld = n if ld is None else ld
    U, V = _padded(u0, ld), _padded(v0, ld)
    keep, d_load, ld_load, stride = _loads(loads, n, ld)
    if d_load is not None and stride:
        d_load += 8 * 2 * first * stride
    kin, pot = c.g.lod_irk_wave_steps(f, scheme, sym, mass, cols, dt, n_steps, U.data_ptr(), V.data_ptr(), n_rhs=n, member=member,
                                      ld_u=ld, ld_v=ld, d_load=d_load, ld_load=ld_load, load_stage_stride=stride, damp_mass=dm,
                                      damp_stiff=ds, energies=energies, d_damping=dmat if damping else None)
    _sync()
    return U, V, kin, pot


def _solve(f, Br, Bi, n, K=None, first=0, shared=False):
    K = f.n_members - first if K is None else K
    ur, ui = _nan(Br.shape[0], K * n), _nan(Br.shape[0], K * n)
    f.solve_complex(Br.data_ptr(), None if Bi is None else Bi.data_ptr(), ur.data_ptr(), ui.data_ptr(), n_rhs=n, first_member=first,
                    n_members=K, shared_rhs=shared, ld_rhs=Br.shape[1], ld_u=K * n)
    _sync()
    return ur, ui


def _z(ur, ui):
    return ur.cpu().numpy() + 1j * ui.cpu().numpy()


def _words(ur, ui):
    return np.stack([_bits(ur), _bits(ui)])


def _info_words(f, k):
    i, m = f.inertia(k), f.member_info(k)
    assert (i.n_negative, i.n_positive) == (-1, -1)
    return np.array([i.min_abs_pivot, i.max_abs_pivot, i.norm_matrix, i.norm_factor, m.min_pivot, m.max_pivot]).tobytes()


def _data(c, seed, levels):
    rng = np.random.default_rng(seed)
    n = 17
    u0 = rng.uniform(-1.0, 1.0, (c.nrow, n))
    v0 = np.sqrt(c.lam_h[len(c.lam_h) // 2]) * rng.uniform(-1.0, 1.0, (c.nrow, n))
    const = c.A @ rng.uniform(-1.0, 1.0, (c.nrow, n))
    per = np.array([c.A @ rng.uniform(-1.0, 1.0, (c.nrow, n)) for _ in range(levels)])
    return u0, v0, {"none": None, "constant": const, "distinct": per}


def _cut(loads, n):
    return None if loads is None else loads[..., :n]


def test_conditions_on_the_sponge_matrix(so):
    for name in sc.CASES:
        c = sc.sponge_case(so, name)                                    # asserts symmetry and semi-definiteness
        print("%s: %d of %d rows of D are zero, sigma_max %.6e" % (name, len(c.zero_rows), c.nrow, sc.sigma_max(c.lam_h)))
    assert len(sc.sponge_case(so, "morton16").zero_rows) >= 1
    import slod_amd
    c = sc.sponge_case(so, "rowmajor")
    assert np.allclose(slod_amd.sponge_profile(c.g.NE, sc.WIDTH, sc.sigma_max(c.lam_h)), c.sigma, rtol=1e-14, atol=0.0)


# ---- 1. NULL damping gives the old words

@pytest.mark.parametrize("name", ["rowmajor", "s2"])
def test_null_damping_gives_the_old_words(so, name):
    torch, dev = _torch()
    c = sc.sponge_case(so, name)
    g, lib, n = c.g, c.g.lib, 3
    sym, mass, _, cols = _mats(c)
    u0, v0, loads = _data(c, 801, STEPS + 1)
    L = _dev(loads["distinct"][:, :, :n])
    dm, ds = sc.sponge_dampings(c.lam_h)[1][1:]
    dt = 0.7 / np.sqrt(c.lam_h[0])
    fM = g.lod_factor(mass, cols)
    S = _nan(c.sym.numel())
    g.lod_matrix_combine(1.0 + 0.5 * dt * dm, mass, 0.25 * dt * dt + 0.5 * dt * ds, sym, S.data_ptr())
    fS = g.lod_factor(S.data_ptr(), cols)

    def fresh():
        return _dev(u0[:, :n]), _dev(v0[:, :n]), _nan(c.nrow, n)

    # the initial acceleration, CG and on the factor of M
    U, V, A = fresh()
    its, res = g.lod_newmark_accel(sym, mass, cols, U.data_ptr(), V.data_ptr(), A.data_ptr(), n_rhs=n, d_load=L[0].data_ptr(),
                                   damp_mass=dm, damp_stiff=ds)
    U2, V2, A2 = fresh()
    its2, res2 = np.zeros(n, dtype=np.intc), np.zeros(n)
    rc = lib.slod_lod_newmark_accel_damped(g.h, sym, mass, None, cols, dm, ds, n, U2.data_ptr(), n, V2.data_ptr(), n, L[0].data_ptr(), n,
                                           A2.data_ptr(), n, 1e-12, 2000, its2.ctypes.data_as(IP), res2.ctypes.data_as(DP))
    _sync()
    assert rc == its.max() and np.array_equal(_bits(A), _bits(A2)) and np.array_equal(its, its2) and res.tobytes() == res2.tobytes()
    g.lod_newmark_accel_direct(fM, sym, mass, cols, U.data_ptr(), V.data_ptr(), A.data_ptr(), n_rhs=n, d_load=L[0].data_ptr(),
                               damp_mass=dm, damp_stiff=ds)
    g._check(lib.slod_lod_newmark_accel_damped_direct(g.h, fM.f, sym, mass, None, cols, dm, ds, n, U2.data_ptr(), n, V2.data_ptr(), n,
                                                      L[0].data_ptr(), n, A2.data_ptr(), n))
    _sync()
    assert np.array_equal(_bits(A), _bits(A2)) and bool(torch.isfinite(A).all())
    a0 = A.clone()
    # the steps, CG and on the factor of S
    shape = (STEPS + 1, n)
    for direct in (False, True):
        U, V = fresh()[:2]
        A = a0.clone()
        kw = dict(n_rhs=n, d_load=L.data_ptr(), load_step_stride=c.nrow * n, damp_mass=dm, damp_stiff=ds)
        U2, V2, A2 = U.clone(), V.clone(), A.clone()
        k2, p2 = np.zeros(shape), np.zeros(shape)
        if direct:
            kin, pot = g.lod_newmark_steps_direct(fS, sym, mass, cols, dt, STEPS, U.data_ptr(), V.data_ptr(), A.data_ptr(), **kw)
            g._check(lib.slod_lod_newmark_steps_damped_direct(g.h, fS.f, sym, mass, None, cols, dt, 0.25, 0.5, dm, ds, STEPS, n,
                                                              U2.data_ptr(), n, V2.data_ptr(), n, A2.data_ptr(), n, L.data_ptr(), n,
                                                              c.nrow * n, k2.ctypes.data_as(DP), p2.ctypes.data_as(DP)))
        else:
            its, res, kin, pot = g.lod_newmark_steps(sym, mass, cols, dt, STEPS, U.data_ptr(), V.data_ptr(), A.data_ptr(), **kw)
            its2, res2 = np.zeros(STEPS, dtype=np.intc), np.zeros(STEPS)
            rc = lib.slod_lod_newmark_steps_damped(g.h, sym, mass, None, cols, dt, 0.25, 0.5, dm, ds, STEPS, n, U2.data_ptr(), n,
                                                   V2.data_ptr(), n, A2.data_ptr(), n, L.data_ptr(), n, c.nrow * n, 1e-12, 2000,
                                                   its2.ctypes.data_as(IP), res2.ctypes.data_as(DP), k2.ctypes.data_as(DP),
                                                   p2.ctypes.data_as(DP))
            assert rc == its.max() and np.array_equal(its, its2) and res.tobytes() == res2.tobytes()
        _sync()
        for a, b in ((U, U2), (V, V2), (A, A2)):
            assert np.array_equal(_bits(a), _bits(b)) and bool(torch.isfinite(a).all()), direct
        assert kin.tobytes() == k2.tobytes() and pot.tobytes() == p2.tobytes()
    fM.close()
    fS.close()
    # the IRK wave stepper on the two-term factor
    stage = np.concatenate([loads["distinct"], loads["distinct"][:2]])[:2 * STEPS]
    for label, scheme in sc.SCHEMES:
        a, b = g.lod_irk_coefficients(scheme, 2, dt, dm, ds)
        f = g.lod_factor_zldl(sym, mass, cols, [a], [b])
        U, V, kin, pot = _irk_run(c, f, scheme, dt, STEPS, u0[:, :n], v0[:, :n], dm, ds, stage, damping=False)
        U2, V2 = _dev(u0[:, :n]), _dev(v0[:, :n])
        Lt = _dev(stage[:, :, :n])
        k2, p2 = np.zeros(shape), np.zeros(shape)
        g._check(lib.slod_lod_irk_wave_steps_damped_direct(g.h, f.f, 0, scheme, sym, mass, None, cols, dt, dm, ds, STEPS, n, U2.data_ptr(),
                                                           n, V2.data_ptr(), n, Lt.data_ptr(), n, c.nrow * n, k2.ctypes.data_as(DP),
                                                           p2.ctypes.data_as(DP)))
        _sync()
        assert np.array_equal(_bits(U), _bits(U2)) and np.array_equal(_bits(V), _bits(V2)) and bool(torch.isfinite(U).all()), label
        assert kin.tobytes() == k2.tobytes() and pot.tobytes() == p2.tobytes()
        f.close()
    # the frequency response
    w = np.array(sc.rule_frequencies(c.lam_h))
    rng = np.random.default_rng(802)
    Br, Bi = _dev(rng.uniform(-1.0, 1.0, (c.nrow, n))), _dev(rng.uniform(-1.0, 1.0, (c.nrow, n)))
    ur, ui = _nan(c.nrow, 8 * n), _nan(c.nrow, 8 * n)
    res, growth = g.lod_harmonic_response(sym, mass, cols, w, Br.data_ptr(), Bi.data_ptr(), ur.data_ptr(), ui.data_ptr(), n_rhs=n,
                                          damp_mass=dm, damp_stiff=ds)
    ur2, ui2 = _nan(c.nrow, 8 * n), _nan(c.nrow, 8 * n)
    res2, growth2, q = np.zeros((8, n)), np.zeros(8), np.full((8, n, 5), NAN)
    g._check(lib.slod_lod_harmonic_response_damped(g.h, sym, mass, None, cols, dm, ds, w.ctypes.data_as(DP), 8, Br.data_ptr(),
                                                   Bi.data_ptr(), n, n, ur2.data_ptr(), ui2.data_ptr(), 8 * n, res2.ctypes.data_as(DP),
                                                   growth2.ctypes.data_as(DP), q.ctypes.data_as(DP)))
    assert np.array_equal(_words(ur, ui), _words(ur2, ui2)) and bool(torch.isfinite(ur).all())
    assert res.tobytes() == res2.tobytes() and growth.tobytes() == growth2.tobytes()
    assert (q[:, :, 2] == 0.0).all() and np.isfinite(q).all() and (q[:, :, 0] > 0.0).all()


# ---- 2. Newmark against the dense recursion

@pytest.mark.parametrize("beta", [0.25, 0.0])
@pytest.mark.parametrize("name", sc.CASES)
def test_newmark_against_the_dense_recursion(so, name, beta):
    torch, dev = _torch()
    c = sc.sponge_case(so, name)
    g = c.g
    sym, mass, dmat, cols = _mats(c)
    u0, v0, loads = _data(c, 811, STEPS + 1)
    dt = 0.7 / np.sqrt(c.lam_h[0]) if beta > 0.0 else 1.8 / np.sqrt(c.lam_h[-1])
    fM = g.lod_factor(mass, cols)
    worst = {}
    for dlabel, dm, ds in sc.sponge_dampings(c.lam_h):
        fS = _nm_factor(c, dt, beta, 0.5, dm, ds, ldl=beta == 0.0)        # Cholesky for one beta, LDL^T for the other
        for kind, b in loads.items():
            level = (lambda k: 0.0 * u0) if b is None else (lambda k: b) if b.ndim == 2 else (lambda k: b[k])
            a0 = sc.newmark_accel(c.A, c.M, c.D, u0, v0, level(0), dm, ds)
            us, vs, acs = sc.newmark(c.A, c.M, c.D, dt, beta, 0.5, STEPS, u0, v0, a0, level, dm, ds)
            rk, rp = sc.energies(c.A, c.M, us, vs)
            for n in (1, 3, 17):
                for how in ("direct", "cg"):
                    U, V, A = _dev(u0[:, :n]), _dev(v0[:, :n]), _nan(c.nrow, n)
                    keep, d_load, ld_load, _ = _loads(None if b is None else level(0), n, n)
                    kw = dict(n_rhs=n, d_load=d_load, ld_load=ld_load, damp_mass=dm, damp_stiff=ds, d_damping=dmat)
                    if how == "direct":
                        g.lod_newmark_accel_direct(fM, sym, mass, cols, U.data_ptr(), V.data_ptr(), A.data_ptr(), **kw)
                    else:
                        g.lod_newmark_accel(sym, mass, cols, U.data_ptr(), V.data_ptr(), A.data_ptr(), rel_tol=1e-13,
                                            max_iterations=5000, **kw)
                    _sync()
                    e_a = _rel(_np(A, n), a0[:, :n])
                    kin, pot = _nm_run(c, fS if how == "direct" else None, dt, beta, STEPS, (U, V, A), _cut(b, n), dm, ds, n)
                    errs = [e_a, _rel(_np(U, n), us[-1][:, :n]), _rel(_np(V, n), vs[-1][:, :n]), _rel(_np(A, n), acs[-1][:, :n]),
                            float(max(np.abs(kin - rk[:, :n]).max(), np.abs(pot - rp[:, :n]).max()) / rp[:, :n].max())]
                    assert all(np.isfinite(_np(t, n)).all() for t in (U, V, A))
                    worst[how] = max(worst.get(how, 0.0), *errs)
                    assert max(errs) <= sc.FORWARD, (name, beta, dlabel, kind, n, how, errs)
        if dlabel == "sponge+both":                                      # the word properties, on the factor
            b, n = loads["distinct"], 17
            a0 = _dev(sc.newmark_accel(c.A, c.M, c.D, u0, v0, b[0], dm, ds))

            def fresh(cols_=slice(0, n), ld=None):
                k = u0[:, cols_].shape[1]
                ld = k if ld is None else ld
                return _padded(u0[:, cols_], ld), _padded(v0[:, cols_], ld), _padded(a0.cpu().numpy()[:, cols_], ld)

            two = fresh()
            k2, p2 = _nm_run(c, fS, dt, beta, 2, two, b, dm, ds, n)
            one = fresh()
            ka, pa = _nm_run(c, fS, dt, beta, 1, one, b, dm, ds, n)
            kb, pb = _nm_run(c, fS, dt, beta, 1, one, b, dm, ds, n, first=1)
            for x, y in zip(one, two):
                assert np.array_equal(_bits(x), _bits(y))
            assert np.stack([ka[0], ka[1], kb[1]]).tobytes() == k2.tobytes() and np.stack([pa[0], pa[1], pb[1]]).tobytes() == p2.tobytes()
            for j in (0, 5, 16):                                         # a column equals its own run
                own = fresh(slice(j, j + 1))
                kj, pj = _nm_run(c, fS, dt, beta, 2, own, b[:, :, j:j + 1], dm, ds, 1)
                for x, y in zip(own, two):
                    assert np.array_equal(_bits(x)[:, 0], _bits(y)[:, j]), j
                assert kj[:, 0].tobytes() == k2[:, j].tobytes() and pj[:, 0].tobytes() == p2[:, j].tobytes()
            wide = fresh(ld=n + 3)                                       # a padded ld keeps its NaN
            kw_, pw_ = _nm_run(c, fS, dt, beta, 2, wide, b, dm, ds, n, ld=n + 3)
            for x, y in zip(wide, two):
                assert np.array_equal(_bits(x[:, :n]), _bits(y)) and bool(torch.isnan(x[:, n:]).all())
            assert kw_.tobytes() == k2.tobytes()
            # and the damped call differs from the call without D
            plain = fresh()
            _nm_run(c, fS, dt, beta, 2, plain, b, dm, ds, n, damping=False)
            assert not np.array_equal(_bits(plain[0]), _bits(two[0]))
        fS.close()
    fM.close()
    print("%s beta %.2f, %d steps: worst error against the dense recursion: direct %.3e, CG %.3e of max |reference|"
          % (name, beta, STEPS, worst["direct"], worst["cg"]))


# ---- 3. energy

@pytest.mark.parametrize("name", sc.CASES)
def test_trapezoidal_energy_identity(so, name):
    torch, dev = _torch()
    c = sc.sponge_case(so, name)
    g = c.g
    sym, mass, dmat, cols = _mats(c)
    steps, n = 10, 3
    dt = 0.7 / np.sqrt(c.lam_h[0])
    rng = np.random.default_rng(821)
    u0, v0 = rng.uniform(-1.0, 1.0, (c.nrow, n)), np.sqrt(c.lam_h[0]) * rng.uniform(-1.0, 1.0, (c.nrow, n))
    starts = [("random", u0, v0)]
    if name == "morton16":                                               # a state on the zero rows of D: coupled through A only
        z = np.zeros((c.nrow, n))
        z[c.zero_rows] = rng.uniform(-1.0, 1.0, (len(c.zero_rows), n))
        assert not (c.D @ z).any()
        starts.append(("zero rows", z, np.zeros((c.nrow, n))))
    fM = g.lod_factor(mass, cols)
    for dlabel, dm, ds in sc.sponge_dampings(c.lam_h):
        fS = _nm_factor(c, dt, 0.25, 0.5, dm, ds)
        for slabel, us, vs in starts:
            U, V, A = _dev(us), _dev(vs), _nan(c.nrow, n)
            g.lod_newmark_accel_direct(fM, sym, mass, cols, U.data_ptr(), V.data_ptr(), A.data_ptr(), n_rhs=n, damp_mass=dm,
                                       damp_stiff=ds, d_damping=dmat)
            E, loss = [], []
            for k in range(steps):
                Vold = V.clone()
                kin, pot = _nm_run(c, fS, dt, 0.25, 1, (U, V, A), None, dm, ds, n)
                vbar = 0.5 * (Vold + V)
                q = [g.lod_inner(x, cols, vbar.data_ptr(), vbar.data_ptr(), n_rhs=n) for x in (mass, sym, dmat)]
                _sync()
                loss.append(dt * (dm * q[0] + ds * q[1] + q[2]))
                E += [kin[0] + pot[0]] if k == 0 else []
                E.append(kin[1] + pot[1])
            E, loss = np.array(E), np.array(loss)
            off = float((np.abs((E[1:] - E[:-1]) + loss) / E[0]).max())
            rise = float(((E[1:] - E[:-1]) / E[0]).max())
            print("%s %s %s: energy identity off by %.3e of E_0, largest rise %.3e, E_end / E_0 = %.6f"
                  % (name, dlabel, slabel, off, rise, (E[-1] / E[0]).max()))
            assert (E[1:] <= E[:-1] + 1e-12 * E[0]).all(), (name, dlabel, slabel, rise)
            if slabel == "random":
                assert off <= 1e-8, (name, dlabel, off)
                assert (E[-1] < E[0]).all()
        fS.close()
    fM.close()


# ---- 4. the three-term factor

@pytest.mark.parametrize("name", sc.CASES)
def test_zldl3_against_the_yardstick(so, name):
    c = sc.sponge_case(so, name)
    b, rng = c.hbw, np.random.default_rng(831)
    for label, (dm, ds, freqs) in c.sponge_sweep.items():
        omegas = np.array([w for w, _, _ in freqs])
        alpha, beta = sc.harmonic_coefficients(omegas, dm, ds)
        f = _zfactor3(c, alpha, beta, 1j * omegas)
        assert (f.bad_pivot == -1).all() and f.n_members == 8
        assert (f.info.n, f.info.half_bandwidth, f.info.block) == (c.nrow, b, 16)
        S = [sc.harmonic_system(c.A, c.M, c.D, w, dm, ds) for w in omegas]
        worst = dict(growth=0.0, norm=0.0, eta=0.0, solve=0.0)
        for k, (w, ref, moves) in enumerate(freqs):
            ine = f.inertia(k)
            norm = float(np.abs(S[k]).astype(np.longdouble).sum(axis=1).max())
            d_norm = abs(ine.norm_matrix - norm) / norm
            assert d_norm <= (2 * b + 2) * sc.U, (name, label, k, d_norm)
            assert 0.5 * ref.G <= ine.norm_factor <= 2.0 * ref.G, (name, label, k, ine.norm_factor, ref.G)
            lo, hi = np.abs(ref.d).min(), np.abs(ref.d).max()
            assert max(abs(ine.min_abs_pivot - lo) / lo, abs(ine.max_abs_pivot - hi) / hi) <= 1e-10, (name, label, k)
            worst.update(growth=max(worst["growth"], ine.growth), norm=max(worst["norm"], d_norm))
            if moves:
                print("%s %s: omega %d moved %d times to %.6e" % (name, label, k, moves, w))
        for n in (1, 3, 17):
            hb = rng.uniform(-1.0, 1.0, (c.nrow, n)) + 1j * rng.uniform(-1.0, 1.0, (c.nrow, n))
            x = _z(*_solve(f, _dev(hb.real), _dev(hb.imag), n, shared=True))
            assert np.isfinite(x).all()
            for k, (w, ref, _) in enumerate(freqs):
                xk = x[:, k * n:(k + 1) * n]
                e = sc.zeta(S[k], ref.G, xk, hb)
                assert (e <= sc.ZBOUND * sc.bound(b)).all(), (name, label, k, n, e.max(), sc.ZBOUND * sc.bound(b))
                e_solve = float((np.abs(xk - np.linalg.solve(S[k], hb)).max(axis=0) / np.abs(xk).max(axis=0)).max())
                worst.update(eta=max(worst["eta"], e.max()), solve=max(worst["solve"], e_solve))
                assert e_solve <= sc.FORWARD, (name, label, k, n, e_solve)
        if name == "dense":                                              # the band read back on unit columns
            eye = np.eye(c.nrow)
            X = _z(*_solve(f, _dev(eye), None, c.nrow, shared=True))
            for k in range(8):
                Xk = X[:, k * c.nrow:(k + 1) * c.nrow]
                e = sc.zeta(S[k], freqs[k][1].G, Xk, eye + 0j)
                assert (e <= sc.ZBOUND * sc.bound(b)).all(), (label, k, e.max())
                assert np.abs(Xk - np.linalg.inv(S[k])).max() <= sc.FORWARD * np.abs(Xk).max()
        print("%s %s: growth <= %.3e, norm_matrix off by %.2e; backward error %.3e = %.4f of the bound; forward error %.3e"
              % (name, label, worst["growth"], worst["norm"], worst["eta"], worst["eta"] / (sc.ZBOUND * sc.bound(b)), worst["solve"]))
        f.close()


@pytest.mark.parametrize("name", ["rowmajor", "morton16"])
def test_zldl3_members_and_refusals(so, name):
    import slod_amd
    torch, dev = _torch()
    c = sc.sponge_case(so, name)
    g = c.g
    sym, mass, dmat, cols = _mats(c)
    dm, ds, freqs = c.sponge_sweep["sponge+both"]
    omegas = np.array([freqs[k][0] for k in (1, 7, 4)])
    alpha, beta = sc.harmonic_coefficients(omegas, dm, ds)
    gamma = 1j * omegas
    f = _zfactor3(c, alpha, beta, gamma)
    n = 3
    rng = np.random.default_rng(832)
    Br, Bi = _dev(rng.uniform(-1.0, 1.0, (c.nrow, n))), _dev(rng.uniform(-1.0, 1.0, (c.nrow, n)))
    wide = _words(*_solve(f, Br, Bi, n, shared=True))
    for k in range(3):                                                   # a member alone, and at another position
        fk = _zfactor3(c, alpha[k], beta[k], gamma[k])
        assert _info_words(fk, 0) == _info_words(f, k), k
        assert np.array_equal(_words(*_solve(fk, Br, Bi, n, shared=True)), wide[:, :, k * n:(k + 1) * n]), k
        fk.close()
    order = [2, 0, 1]
    fp = _zfactor3(c, alpha[order], beta[order], gamma[order])
    for j, k in enumerate(order):
        assert _info_words(fp, j) == _info_words(f, k)
        assert np.array_equal(_words(*_solve(fp, Br, Bi, n, K=1, first=j, shared=True)), wide[:, :, k * n:(k + 1) * n])
    fp.close()
    # gamma = 0 gives the words of the two-term factor; a non-zero gamma does not
    f0 = _zfactor3(c, alpha, beta, 0.0 * gamma)
    f2 = g.lod_factor_zldl(sym, mass, cols, alpha, beta)
    assert np.array_equal(_words(*_solve(f0, Br, Bi, n, shared=True)), _words(*_solve(f2, Br, Bi, n, shared=True)))
    assert not np.array_equal(_words(*_solve(f2, Br, Bi, n, shared=True)), wide)
    f0.close()
    f2.close()
    # a zero matrix triple for member 1: its status word and the message
    a0, b0, g0 = alpha.copy(), beta.copy(), gamma.copy()
    a0[1] = b0[1] = g0[1] = 0.0
    assert sc.zldl_reference(sc.system3(c.A, c.M, c.D, 0.0, 0.0, 0.0)).bad == 0
    out, bad = C.c_void_p(1), np.full(3, 7, dtype=np.int32)
    ap, bp, gp = (np.ascontiguousarray(x).view(np.float64) for x in (a0, b0, g0))
    rc = g.lib.slod_lod_factor_create_zldl3(g.h, sym, mass, dmat, cols, ap.ctypes.data_as(DP), bp.ctypes.data_as(DP), gp.ctypes.data_as(DP),
                                            3, bad.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(out))
    msg = g.lib.slod_last_error(g.h).decode()
    assert rc == -5 and out.value is None and list(bad) == [-1, 0, -1], (rc, list(bad))
    assert msg == "slod_lod_factor_create_zldl3: member 1: pivot 0 of %d is zero or not finite (0, 0)" % c.nrow, msg
    with pytest.raises(slod_amd.SlodError) as e:
        _zfactor3(c, a0, b0, g0)
    assert e.value.code == -5 and list(e.value.bad_pivot) == [-1, 0, -1]
    # a real consumer refuses the object
    text = "a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex"
    U0, V0, A0 = (_dev(np.ones((c.nrow, 1))) for _ in range(3))
    calls = {
        "slod_lod_factor_solve": lambda: g._check(g.lib.slod_lod_factor_solve(f.f, U0.data_ptr(), 1, 1, V0.data_ptr(), 1, None)),
        "slod_lod_newmark_steps_direct": lambda: g.lod_newmark_steps_direct(f, sym, mass, cols, 0.01, 1, U0.data_ptr(), V0.data_ptr(),
                                                                            A0.data_ptr()),
        "slod_lod_newmark_steps_damped_direct": lambda: g.lod_newmark_steps_direct(f, sym, mass, cols, 0.01, 1, U0.data_ptr(),
                                                                                   V0.data_ptr(), A0.data_ptr(), d_damping=dmat),
        "slod_lod_newmark_accel_damped_direct": lambda: g.lod_newmark_accel_direct(f, sym, mass, cols, U0.data_ptr(), V0.data_ptr(),
                                                                                   A0.data_ptr(), d_damping=dmat),
    }
    for who, call in calls.items():
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith(who + ": " + text), (who, str(e.value))
    assert bool((U0 == 1.0).all()) and bool((V0 == 1.0).all())
    # and the damped IRK stepper refuses a real factor
    real = g.lod_factor(mass, cols)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_irk_wave_steps(real, "gauss", sym, mass, cols, 0.01, 1, U0.data_ptr(), V0.data_ptr(), d_damping=dmat)
    assert e.value.code == -1 and "slod_lod_irk_wave_steps_damped_direct: takes a complex factor" in str(e.value)
    real.close()
    f.close()


# ---- 5. IRK against the stage system

@pytest.mark.parametrize("name", sc.CASES)
def test_irk_against_the_stage_system(so, name):
    torch, dev = _torch()
    c = sc.sponge_case(so, name)
    u0, v0, loads = _data(c, 841, 2 * STEPS)
    worst, growth = {}, 0.0
    dts = sc.wave_dts(c.lam_h)
    for label, scheme in sc.SCHEMES:
        for dlabel, dm, ds in sc.sponge_dampings(c.lam_h):
            for dt in dts:                                               # the condition first, for every dt
                gy, ref = sc.growth_of(sc.irk_system(c.A, c.M, c.D, scheme, dt, dm, ds), c.perm)
                assert ref.bad < 0 and gy <= sc.GROWTH_CAP, (name, label, dlabel, dt, gy)
                growth = max(growth, gy)
            f = _irk_factor(c, scheme, dts, dm, ds)
            assert (f.bad_pivot == -1).all() and f.n_members == 3
            for m, dt in enumerate(dts):
                for kind, b in loads.items():
                    ru, rv = sc.wave_stage(c.A, c.M, c.D, scheme, dt, STEPS, u0, v0, dm, ds, b)
                    rk, rp = sc.energies(c.A, c.M, ru, rv)
                    for n in (1, 3, 17):
                        U, V, kin, pot = _irk_run(c, f, scheme, dt, STEPS, u0[:, :n], v0[:, :n], dm, ds, _cut(b, n), member=m)
                        gu, gv = _np(U, n), _np(V, n)
                        assert np.isfinite(gu).all() and np.isfinite(gv).all()
                        errs = [_rel(gu, ru[-1][:, :n]), _rel(gv, rv[-1][:, :n]),
                                float(max(np.abs(kin - rk[:, :n]).max(), np.abs(pot - rp[:, :n]).max()) / rp[:, :n].max())]
                        worst[label] = max(worst.get(label, 0.0), *errs)
                        assert max(errs) <= sc.FORWARD, (name, label, dlabel, m, kind, n, errs)
            if dlabel == "sponge+both":                                  # the word properties
                b, n, m, dt = loads["distinct"], 17, 1, dts[1]
                U2, V2, k2, p2 = _irk_run(c, f, scheme, dt, 2, u0, v0, dm, ds, b, member=m)
                Ua, Va, ka, pa = _irk_run(c, f, scheme, dt, 1, u0, v0, dm, ds, b, member=m)
                Ub, Vb, kb, pb = _irk_run(c, f, scheme, dt, 1, _np(Ua, n), _np(Va, n), dm, ds, b, member=m, first=1)
                assert np.array_equal(_bits(Ub), _bits(U2)) and np.array_equal(_bits(Vb), _bits(V2))
                assert np.stack([ka[0], ka[1], kb[1]]).tobytes() == k2.tobytes() and np.stack([pa[0], pa[1], pb[1]]).tobytes() == p2.tobytes()
                for j in (0, 5, 16):
                    Uj, Vj, kj, pj = _irk_run(c, f, scheme, dt, 2, u0[:, j:j + 1], v0[:, j:j + 1], dm, ds, b[:, :, j:j + 1], member=m)
                    assert np.array_equal(_bits(Uj)[:, 0], _bits(U2)[:, j]) and np.array_equal(_bits(Vj)[:, 0], _bits(V2)[:, j]), j
                    assert kj[:, 0].tobytes() == k2[:, j].tobytes() and pj[:, 0].tobytes() == p2[:, j].tobytes()
                Uw, Vw, kw_, _ = _irk_run(c, f, scheme, dt, 2, u0, v0, dm, ds, b, ld=n + 3, member=m)
                assert np.array_equal(_bits(Uw[:, :n]), _bits(U2)) and np.array_equal(_bits(Vw[:, :n]), _bits(V2))
                assert bool(torch.isnan(Uw[:, n:]).all()) and bool(torch.isnan(Vw[:, n:]).all()) and kw_.tobytes() == k2.tobytes()
                fk = _irk_factor(c, scheme, dt, dm, ds)                    # the member alone
                U1, V1, _, _ = _irk_run(c, fk, scheme, dt, 2, u0, v0, dm, ds, b)
                assert np.array_equal(_bits(U1), _bits(U2)) and np.array_equal(_bits(V1), _bits(V2))
                fk.close()
            f.close()
    print("%s damped IRK wave, %d steps: yardstick growth <= %.3f; worst error against the stage system: gauss %.3e, radau %.3e"
          % (name, STEPS, growth, worst["gauss"], worst["radau"]))


# ---- 6. the frequency response

@pytest.mark.parametrize("name", sc.CASES)
def test_harmonic_response_damped(so, name):
    torch, dev = _torch()
    c = sc.sponge_case(so, name)
    g = c.g
    sym, mass, dmat, cols = _mats(c)
    cap = g.lod_row_capacity()
    rng = np.random.default_rng(851)
    hb = rng.uniform(-1.0, 1.0, (c.nrow, 3)) + 1j * rng.uniform(-1.0, 1.0, (c.nrow, 3))
    hb[:, 0] = c.M @ c.X[:, 0]                                           # the first mode's load, real
    Br, Bi = _dev(hb.real), _dev(hb.imag)
    for label, (dm, ds, freqs) in c.sponge_sweep.items():
        w = np.array([x for x, _, _ in freqs])
        alpha, beta = sc.harmonic_coefficients(w, dm, ds)
        worst = dict(solve=0.0, q=0.0, power=0.0, res=0.0, growth=0.0)
        for n in (1, 3):
            ur, ui = _nan(c.nrow, 8 * n + 2), _nan(c.nrow, 8 * n + 2)
            res, growth, q = g.lod_harmonic_response(sym, mass, cols, w, Br.data_ptr(), Bi.data_ptr() if n > 1 else None, ur.data_ptr(),
                                                     ui.data_ptr(), n_rhs=n, damp_mass=dm, damp_stiff=ds, ld_load=3, ld_u=8 * n + 2,
                                                     d_damping=dmat)
            assert bool(torch.isnan(ur[:, 8 * n:]).all()) and bool(torch.isnan(ui[:, 8 * n:]).all())
            assert res.shape == (8, n) and growth.shape == (8,) and q.shape == (8, n, 5)
            load = hb[:, :n] if n > 1 else hb[:, :1].real + 0j
            got, x = _words(ur[:, :8 * n], ui[:, :8 * n]), _z(ur[:, :8 * n], ui[:, :8 * n])
            assert np.isfinite(x).all()
            f = _zfactor3(c, alpha, beta, 1j * w)                          # the words of create_zldl3 + solve_complex
            assert np.array_equal(_words(*_solve(f, Br[:, :n].contiguous(), Bi[:, :n].contiguous() if n > 1 else None, n, shared=True)), got)
            assert growth.tobytes() == np.array([f.inertia(k).growth for k in range(8)]).tobytes()
            f.close()
            for k in range(8):
                S = sc.harmonic_system(c.A, c.M, c.D, w[k], dm, ds)
                xk = x[:, k * n:(k + 1) * n]
                e_solve = float((np.abs(xk - np.linalg.solve(S, load)).max(axis=0) / np.abs(xk).max(axis=0)).max())
                assert e_solve <= sc.FORWARD, (name, label, n, k, e_solve)
                r = load.astype(np.clongdouble) - S.astype(np.clongdouble) @ xk.astype(np.clongdouble)
                true = np.array(np.sqrt((np.abs(r) ** 2).sum(axis=0)) / np.linalg.norm(load, axis=0), dtype=np.float64)
                room = 64 * sc.U * (np.abs(S).sum(axis=1).max() * np.linalg.norm(xk, axis=0) / np.linalg.norm(load, axis=0) + 1.0)
                assert (np.abs(res[k] - true) <= np.maximum(1e-6 * true, room)).all(), (name, label, n, k, res[k], true)
                model, mag = sc.quantities(c.A, c.M, c.D, xk, load)
                bars = np.array((c.nrow + cap * c.s + 4) * sc.U * mag, dtype=np.float64)
                off = np.array(np.abs(q[k].astype(np.longdouble) - model), dtype=np.float64)
                assert (off <= bars).all(), (name, label, n, k, off, bars)
                ub = np.abs(q[k, :, 3] + 1j * q[k, :, 4])
                power = w[k] * (dm * q[k, :, 0] + ds * q[k, :, 1] + q[k, :, 2])
                assert (np.abs(power - q[k, :, 4]) <= 1e-8 * ub).all(), (name, label, n, k, power, q[k, :, 4])
                worst.update(solve=max(worst["solve"], e_solve), q=max(worst["q"], float((off / bars).max())),
                             power=max(worst["power"], float((np.abs(power - q[k, :, 4]) / ub).max())), res=max(worst["res"], res[k].max()),
                             growth=max(worst["growth"], growth[k]))
        print("%s %s: growth <= %.3e, residual <= %.3e, forward error %.3e, quantities at %.3f of their bars, power identity off by %.3e"
              % (name, label, worst["growth"], worst["res"], worst["solve"], worst["q"], worst["power"]))
    # a zero load column: u = 0, residual 0 and five exact zeros
    Z = torch.zeros((c.nrow, 2), dtype=torch.float64, device=dev)
    Z[:, 1] = Br[:, 1]
    ur, ui = _nan(c.nrow, 4), _nan(c.nrow, 4)
    res, _, q = g.lod_harmonic_response(sym, mass, cols, w[:2], Z.data_ptr(), None, ur.data_ptr(), ui.data_ptr(), n_rhs=2, damp_mass=dm,
                                        damp_stiff=ds, d_damping=dmat)
    assert bool((ur[:, 0::2] == 0.0).all()) and bool((ui[:, 0::2] == 0.0).all()) and (res[:, 0] == 0.0).all() and (res[:, 1] > 0.0).all()
    assert (q[:, 0, :] == 0.0).all() and (q[:, 1, :3] > 0.0).all()


# ---- 7. record and source

def test_record_and_source_in_the_damped_loops(so):
    import lod_source_cases as src_cases
    torch, dev = _torch()
    c = sc.sponge_case(so, "rowmajor")
    g = c.g
    sym, mass, dmat, cols = _mats(c)
    dm, ds = sc.sponge_dampings(c.lam_h)[1][1:]
    steps, n, nsrc = 4, 2, 6
    dt = 0.7 / np.sqrt(c.lam_h[0])
    recv = g.lod_receivers(src_cases.six(g.cfg.n_subdivisions, g.N, c.s), c.b.data_ptr(), c.stride)
    src = g.lod_sources(recv)
    nr = recv.n_recv
    rng = np.random.default_rng(861)
    u0, v0, a0 = (rng.uniform(-1.0, 1.0, (c.nrow, n)) for _ in range(3))

    def observe(x):
        y = _nan(nr, n)
        recv.observe(x.data_ptr(), y.data_ptr(), n_rhs=n)
        _sync()
        return _bits(y)

    def materialise(sig):
        L = _nan(sig.shape[0], c.nrow, n)
        for j in range(sig.shape[0]):
            src.inject(sig[j].data_ptr(), L[j].data_ptr(), n_rhs=n)
        _sync()
        return L

    fS = _nm_factor(c, dt, 0.25, 0.5, dm, ds)
    a, b = g.lod_irk_coefficients("gauss", 2, dt, dm, ds)
    fZ = _zfactor3(c, [a], [b], [g.lod_irk_damping_coefficient("gauss", dt)])
    for kind in ("newmark", "irk"):
        ns = steps + 1 if kind == "newmark" else 2 * steps
        per = 1 if kind == "newmark" else 2
        sig = _dev(rng.uniform(-1.0, 1.0, (ns, nsrc, n)))
        L = materialise(sig)

        def run(state, n_steps, armed, first=0):
            if armed:
                g.lod_time_source(src, sig.data_ptr(), n_samples=ns, ld_signal=n, sample_stride=nsrc * n)
                d_load, stride = None, 0
            else:
                d_load, stride = L.data_ptr() + 8 * first * per * c.nrow * n, c.nrow * n
            if kind == "newmark":
                out = g.lod_newmark_steps_direct(fS, sym, mass, cols, dt, n_steps, state[0].data_ptr(), state[1].data_ptr(),
                                                 state[2].data_ptr(), n_rhs=n, d_load=d_load, ld_load=n, load_step_stride=stride,
                                                 damp_mass=dm, damp_stiff=ds, d_damping=dmat)
            else:
                out = g.lod_irk_wave_steps(fZ, "gauss", sym, mass, cols, dt, n_steps, state[0].data_ptr(), state[1].data_ptr(), n_rhs=n,
                                           d_load=d_load, ld_load=n, load_stage_stride=stride, damp_mass=dm, damp_stiff=ds,
                                           d_damping=dmat)
            _sync()
            return out

        # the un-armed call on materialised loads, step by step, observed
        st = [_dev(u0), _dev(v0), _dev(a0)]
        want = [(observe(st[0]), observe(st[1]))]
        for k in range(steps):
            run(st, 1, False, first=k)
            want.append((observe(st[0]), observe(st[1])))
        whole = [_dev(u0), _dev(v0), _dev(a0)]
        e_plain = run(whole, steps, False)
        for x, y in zip(whole, st):
            assert np.array_equal(_bits(x), _bits(y)), kind
        # the armed call
        trace = _nan(steps + 1, 2, nr, n)
        g.lod_time_record(recv, trace.data_ptr(), capacity=steps + 1, what=3, ld_trace=n)
        armed = [_dev(u0), _dev(v0), _dev(a0)]
        e_armed = run(armed, steps, True)
        for x, y in zip(armed, whole):
            assert np.array_equal(_bits(x), _bits(y)) and bool(torch.isfinite(x).all()), kind
        for p, q_ in zip(e_plain, e_armed):
            assert p.tobytes() == q_.tobytes()
        tw = _bits(trace)
        for j in range(steps + 1):
            assert np.array_equal(tw[j, 0], want[j][0]) and np.array_equal(tw[j, 1], want[j][1]), (kind, j)
        # and the source did drive the loop
        quiet = [_dev(u0), _dev(v0), _dev(a0)]
        L.zero_()
        run(quiet, steps, False)
        assert not np.array_equal(_bits(quiet[0]), _bits(whole[0]))
    fS.close()
    fZ.close()
    src.close()
    recv.close()


# ---- 8. the mirror and the driver

def _driver(*args):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "dealii-slod_amd", "bin", "main_Diffusion")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", os.path.join(root, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([binary, "3", "4", "1", "1"] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_driver_sponge_matches_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --wave 8 DT --direct --sponge 0.25 S, the same with --irk gauss, and --harmonic 5 W0 W1
    --sponge 0.25 S (the driver's coefficient Alpha(1, 100, 3), srand(1); f = 1, from rest) print the numbers of the Python
    path to the digits printed; kinetic + potential - work, zero at rest, does not rise under the constant load."""
    import scipy.linalg as sl
    import slod_amd
    from lod_cases import _build, _mass, _rows_to_dense, _symmetrize
    torch, dev = _torch()
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    g = c.g
    c.mvalues, _ = _mass(c)
    c.sym = _symmetrize(c)
    hcols = c.cols.cpu().numpy().view(np.uint32)
    lam = sl.eigh(_rows_to_dense(g, c.sym.cpu().numpy(), hcols, 1), _rows_to_dense(g, c.mvalues.cpu().numpy(), hcols, 1),
                  eigvals_only=True)
    w1 = float(np.sqrt(lam[0]))
    width, smax, steps, dt = 0.25, 4.0 * w1, 8, 0.7 / w1
    sigma = torch.from_numpy(slod_amd.sponge_profile(g.NE, width, smax)).to(dev)
    c.dvalues, _ = _mass(c, sigma)
    D = _rows_to_dense(g, c.dvalues.cpu().numpy(), hcols, 1)
    sym, mass, dmat, cols = _mats(c)
    fld = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, fld.data_ptr())
    rhs = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
    g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, fld.data_ptr(), rhs.data_ptr())
    b = rhs.cpu().numpy()[:, 0]
    sponge_line = "sponge: width = %g, sigma_max = %.12e, zero coarse rows of D = %d" % (width, smax, int((~D.any(axis=1)).sum()))

    def check_wave(out, step):
        assert sponge_line in out, out
        lines = re.findall(r"^wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", out, re.M)
        assert [m[0] for m in lines] == [str(k + 1) for k in range(steps)], out
        total = [0.0]
        for k in range(steps):
            kin, pot, u = step()
            work = 0.0
            for x, y in zip(u, b):                                       # the driver's sum, in its order
                work += x * y
            assert lines[k][1:] == ("%.12e" % kin, "%.12e" % pot, "%.12e" % work), (k, lines[k])
            total.append(float(lines[k][1]) + float(lines[k][2]) - float(lines[k][3]))
        total = np.array(total)
        assert (total[1:] <= total[:-1] + 1e-10 * np.abs(total).max()).all() and total[-1] < 0.0, total

    # Newmark on the factors
    out = _driver("--wave", str(steps), repr(dt), "--direct", "--sponge", repr(width), repr(smax))
    fM, fS = g.lod_factor(mass, cols), _nm_factor(c, dt, 0.25, 0.5, 0.0, 0.0)
    U, V, A = (torch.zeros_like(rhs) for _ in range(3))
    g.lod_newmark_accel_direct(fM, sym, mass, cols, U.data_ptr(), V.data_ptr(), A.data_ptr(), d_load=rhs.data_ptr(), d_damping=dmat)

    def nm_step():
        kin, pot = g.lod_newmark_steps_direct(fS, sym, mass, cols, dt, 1, U.data_ptr(), V.data_ptr(), A.data_ptr(),
                                              d_load=rhs.data_ptr(), d_damping=dmat)
        return kin[1, 0], pot[1, 0], U.cpu().numpy()[:, 0]
    check_wave(out, nm_step)
    fM.close()
    fS.close()
    # Gauss IRK
    out = _driver("--wave", str(steps), repr(dt), "--irk", "gauss", "--sponge", repr(width), repr(smax))
    f = _irk_factor(c, "gauss", dt, 0.0, 0.0)
    U2, V2 = torch.zeros_like(rhs), torch.zeros_like(rhs)

    def irk_step():
        kin, pot = g.lod_irk_wave_steps(f, "gauss", sym, mass, cols, dt, 1, U2.data_ptr(), V2.data_ptr(), d_load=rhs.data_ptr(),
                                        d_damping=dmat)
        return kin[1, 0], pot[1, 0], U2.cpu().numpy()[:, 0]
    check_wave(out, irk_step)
    f.close()
    # the frequency sweep
    K, w0, wK = 5, 0.5 * w1, 2.0 * w1
    out = _driver("--harmonic", str(K), repr(w0), repr(wK), "--sponge", repr(width), repr(smax))
    assert sponge_line in out, out
    lines = re.findall(r"^harmonic (\d+): omega = (\S+), growth = (\S+), relative residual = (\S+), amplitude = (\S+), power = (\S+)$",
                       out, re.M)
    assert [int(m[0]) for m in lines] == list(range(1, K + 1)), out
    omegas = np.array([w0 + k * ((wK - w0) / (K - 1)) for k in range(K)])
    ur, ui = _nan(c.nrow, K), _nan(c.nrow, K)
    res, growth, q = g.lod_harmonic_response(sym, mass, cols, omegas, rhs.data_ptr(), None, ur.data_ptr(), ui.data_ptr(), d_damping=dmat)
    amp, power = np.sqrt(q[:, 0, 0]), 0.5 * omegas * (0.0 * q[:, 0, 0] + 0.0 * q[:, 0, 1] + q[:, 0, 2])
    for k, m in enumerate(lines):
        want = ("%.12e" % omegas[k], "%.6e" % growth[k], "%.6e" % res[k, 0], "%.12e" % amp[k], "%.12e" % power[k])
        assert tuple(m[1:]) == want, (k, m, want)
    assert (power > 0.0).all()
