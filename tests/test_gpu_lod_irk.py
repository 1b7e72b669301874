"""GPU tests of the two-stage implicit Runge-Kutta steppers on the LOD space (slod_lod_irk_coefficients,
slod_lod_irk_heat_steps_direct, slod_lod_irk_wave_steps_direct): one complex solve per step on a member of the complex
banded LDL^T, against the undiagonalised stage system in numpy and the Pade stability functions of lod_irk_cases.py
(checked on the CPU by test_lod_irk_reference.py), and against itself as 64-bit words.

Cases: the four of test_gpu_lod_ldl.py with their real sym(A) and M (dense 16 rows, rowmajor 25, s2 128, morton16 256),
both schemes at the three dt of the rule for heat and for wave, the wave undamped and at the three dampings of
lod_harmonic_cases.py.  The growth cap is asserted on the yardstick before the library is called.  Bars: 1e-8 of
max |reference| for states and energies (FORWARD, the project's bar against a dense reference); for a single mode 1e-8 of
the mode's start, max |x_j| (and sqrt(lam_j) max |x_j| for v), because R(-lam_j dt)^k itself may be far below 1e-8.
The figures the tests print are recorded in DESIGN section 6.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_irk_cases as ic
from lod_cases import NAN, _bits, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
STEPS = 3
REFUSED = "takes a complex factor (slod_lod_factor_create_zldl)"


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _padded(a, ld):
    """[rows][ld] on the device, NaN beyond the columns of a."""
    torch, dev = _torch()
    t = torch.full((a.shape[0], ld), NAN, dtype=torch.float64, device=dev)
    t[:, :a.shape[1]] = _dev(a)
    return t


def _ptrs(c):
    return c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr()


def _factor(c, scheme, order, dts, dm=0.0, ds=0.0):
    """One member per dt."""
    pairs = [c.g.lod_irk_coefficients(scheme, order, dt, dm, ds) for dt in np.atleast_1d(dts)]
    sym, mass, cols = _ptrs(c)
    return c.g.lod_factor_zldl(sym, mass, cols, [p[0] for p in pairs], [p[1] for p in pairs])


def _load_args(loads, n, ld):
    """(tensor kept alive, d_load, ld_load, stride) for None, a constant [rows][>= n] or stage loads [2 steps][rows][>= n]."""
    if loads is None:
        return None, None, None, 0
    if loads.ndim == 2:
        t = _padded(loads[:, :n], ld)
        return t, t.data_ptr(), ld, 0
    torch, dev = _torch()
    t = torch.full((loads.shape[0], loads.shape[1], ld), NAN, dtype=torch.float64, device=dev)
    t[:, :, :n] = _dev(loads[:, :, :n])
    return t, t.data_ptr(), ld, loads.shape[1] * ld


def _heat(c, f, scheme, dt, steps, u0, loads=None, ld=None, member=0):
    """The library's heat run on the columns of u0; returns the device state [rows][ld]."""
    torch, dev = _torch()
    n = u0.shape[1]
    ld = n if ld is None else ld
    U = _padded(u0, ld)
    keep, d_load, ld_load, stride = _load_args(loads, n, ld)
    sym, _, cols = _ptrs(c)
    c.g.lod_irk_heat_steps(f, scheme, sym, cols, dt, steps, U.data_ptr(), n_rhs=n, member=member, ld_u=ld, d_load=d_load,
                           ld_load=ld_load, load_stage_stride=stride)
    torch.cuda.synchronize()
    return U


def _wave(c, f, scheme, dt, steps, u0, v0, dm=0.0, ds=0.0, loads=None, ld=None, member=0, energies=True):
    torch, dev = _torch()
    n = u0.shape[1]
    ld = n if ld is None else ld
    U, V = _padded(u0, ld), _padded(v0, ld)
    keep, d_load, ld_load, stride = _load_args(loads, n, ld)
    sym, mass, cols = _ptrs(c)
    kin, pot = c.g.lod_irk_wave_steps(f, scheme, sym, mass, cols, dt, steps, U.data_ptr(), V.data_ptr(), n_rhs=n, member=member,
                                      ld_u=ld, ld_v=ld, d_load=d_load, ld_load=ld_load, load_stage_stride=stride, damp_mass=dm,
                                      damp_stiff=ds, energies=energies)
    torch.cuda.synchronize()
    return U, V, kin, pot


def _np(t, n):
    return t.cpu().numpy()[:, :n]


def _check_growth(c, f, scheme, order, dt, dm=0.0, ds=0.0, member=0):
    """The condition on the yardstick, then the header's promise for norm_factor.  Returns the library's growth."""
    gy, ref = ic.growth(c.A, c.M, scheme, order, dt, dm, ds, c.perm)
    assert gy <= ic.GROWTH_CAP, (scheme, order, dt, dm, ds, gy)
    if f is None:
        return gy
    ine = f.inertia(member)
    assert 0.5 * ref.G <= ine.norm_factor <= 2.0 * ref.G, (scheme, order, dt, ine.norm_factor, ref.G)
    return ine.growth


def _data(c, seed):
    """17 columns of state, velocity, a constant load and stage loads of the size of A u."""
    rng = np.random.default_rng(seed)
    n = 17
    u0 = rng.uniform(-1.0, 1.0, (c.nrow, n))
    v0 = np.sqrt(c.lam_h[len(c.lam_h) // 2]) * rng.uniform(-1.0, 1.0, (c.nrow, n))
    const = c.A @ rng.uniform(-1.0, 1.0, (c.nrow, n))
    stage = np.array([c.A @ rng.uniform(-1.0, 1.0, (c.nrow, n)) for _ in range(2 * STEPS)])
    return u0, v0, {"none": None, "constant": const, "stage": stage}


def _cut(loads, n):
    return None if loads is None else loads[..., :n]


# ---- against the dense yardstick

@pytest.mark.parametrize("name", ic.CASES)
def test_heat_against_the_stage_system(so, name):
    c = ic.irk_case(so, name)
    u0, _, loads = _data(c, 701)
    worst, growth = {}, 0.0
    for label, scheme in ic.SCHEMES:
        dts = ic.heat_dts(c.lam_h)
        for dt in dts:                                                   # the condition first, for every dt
            _check_growth(c, None, scheme, 1, dt)
        f = _factor(c, scheme, 1, dts)
        assert (f.bad_pivot == -1).all() and f.n_members == 3
        for m, dt in enumerate(dts):
            growth = max(growth, _check_growth(c, f, scheme, 1, dt, member=m))
            for kind, b in loads.items():
                ref = ic.heat_stage(c.A, c.M, scheme, dt, STEPS, u0, b)[-1]
                for n in (1, 3, 17):
                    got = _np(_heat(c, f, scheme, dt, STEPS, u0[:, :n], _cut(b, n), member=m), n)
                    assert np.isfinite(got).all()
                    e = float(np.abs(got - ref[:, :n]).max() / np.abs(ref[:, :n]).max())
                    worst[label] = max(worst.get(label, 0.0), e)
                    assert e <= ic.FORWARD, (name, label, m, kind, n, e)
        f.close()
    print("%s heat, %d steps: growth <= %.3f; worst error against the stage system: gauss %.3e, radau %.3e of max |u|"
          % (name, STEPS, growth, worst["gauss"], worst["radau"]))


@pytest.mark.parametrize("name", ic.CASES)
def test_wave_against_the_stage_system(so, name):
    c = ic.irk_case(so, name)
    u0, v0, loads = _data(c, 702)
    worst, growth = {}, 0.0
    for label, scheme in ic.SCHEMES:
        dts = ic.wave_dts(c.lam_h)
        for dlabel, dm, ds in ic.wave_dampings(c.lam_h):
            for dt in dts:
                _check_growth(c, None, scheme, 2, dt, dm, ds)
            f = _factor(c, scheme, 2, dts, dm, ds)
            assert (f.bad_pivot == -1).all()
            for m, dt in enumerate(dts):
                growth = max(growth, _check_growth(c, f, scheme, 2, dt, dm, ds, member=m))
                for kind, b in loads.items():
                    ru, rv = ic.wave_stage(c.A, c.M, scheme, dt, STEPS, u0, v0, dm, ds, b)
                    rk = 0.5 * np.einsum("kic,ij,kjc->kc", rv, c.M, rv)
                    rp = 0.5 * np.einsum("kic,ij,kjc->kc", ru, c.A, ru)
                    for n in (1, 3, 17):
                        U, V, kin, pot = _wave(c, f, scheme, dt, STEPS, u0[:, :n], v0[:, :n], dm, ds, _cut(b, n), member=m)
                        gu, gv = _np(U, n), _np(V, n)
                        assert np.isfinite(gu).all() and np.isfinite(gv).all()
                        eu = float(np.abs(gu - ru[-1][:, :n]).max() / np.abs(ru[-1][:, :n]).max())
                        ev = float(np.abs(gv - rv[-1][:, :n]).max() / np.abs(rv[-1][:, :n]).max())
                        ee = float(max(np.abs(kin - rk[:, :n]).max(), np.abs(pot - rp[:, :n]).max()) / rp[:, :n].max())
                        for key, e in (("u", eu), ("v", ev), ("E", ee)):
                            worst[label, key] = max(worst.get((label, key), 0.0), e)
                        assert max(eu, ev, ee) <= ic.FORWARD, (name, label, dlabel, m, kind, n, eu, ev, ee)
            f.close()
    print("%s wave, %d steps: growth <= %.3f; worst error against the stage system (u, v, energies): gauss %.3e %.3e %.3e, "
          "radau %.3e %.3e %.3e" % (name, STEPS, growth, *[worst[l, k] for l in ("gauss", "radau") for k in ("u", "v", "E")]))


# ---- single modes against the stability function

@pytest.mark.parametrize("name", ic.CASES)
def test_modes_through_the_library(so, name):
    c = ic.irk_case(so, name)
    lam, nrow = c.lam_h, c.nrow
    js = [0, nrow // 2, nrow - 1]
    X = c.X[:, js]
    scale = np.abs(X).max(axis=0)
    worst = {"heat": 0.0, "wave": 0.0}
    for label, scheme in ic.SCHEMES:
        dts = ic.heat_dts(lam)
        f = _factor(c, scheme, 1, dts)
        for m, dt in enumerate(dts):
            got = _np(_heat(c, f, scheme, dt, STEPS, X, member=m), 3)
            want = X * np.array([ic.stability(scheme, -lam[j] * dt) ** STEPS for j in js])
            e = float((np.abs(got - want).max(axis=0) / scale).max())
            worst["heat"] = max(worst["heat"], e)
            assert e <= ic.FORWARD, (name, label, "heat", m, e)
        f.close()
        dts = ic.wave_dts(lam)
        for dlabel, dm, ds in ic.wave_dampings(lam):
            f = _factor(c, scheme, 2, dts, dm, ds)
            for m, dt in enumerate(dts):
                w = np.sqrt(lam[js])
                U, V, _, _ = _wave(c, f, scheme, dt, STEPS, X, X * w, dm, ds, member=m, energies=False)
                for k, j in enumerate(js):
                    y = np.linalg.matrix_power(ic.wave_amplification(scheme, dt, lam[j], dm, ds), STEPS) @ np.array([1.0, w[k]])
                    eu = float(np.abs(_np(U, 3)[:, k] - y[0] * X[:, k]).max() / scale[k])
                    ev = float(np.abs(_np(V, 3)[:, k] - y[1] * X[:, k]).max() / (w[k] * scale[k]))
                    worst["wave"] = max(worst["wave"], eu, ev)
                    assert max(eu, ev) <= ic.FORWARD, (name, label, dlabel, m, j, eu, ev)
            f.close()
    print("%s modes 0, n/2, n-1 against the stability function after %d steps: heat %.3e, wave %.3e of the start"
          % (name, STEPS, worst["heat"], worst["wave"]))


# ---- what each scheme is for

@pytest.mark.parametrize("name", ic.CASES)
def test_gauss_conserves_the_energy_of_the_undamped_wave(so, name):
    c = ic.irk_case(so, name)
    lam, steps = c.lam_h, 10
    dt = 0.7 / np.sqrt(lam[0])                                            # the step of the trapezoidal test
    rng = np.random.default_rng(703)
    u0, v0 = rng.uniform(-1.0, 1.0, (c.nrow, 3)), np.zeros((c.nrow, 3))
    f = _factor(c, ic.GAUSS, 2, dt)
    _, _, kin, pot = _wave(c, f, ic.GAUSS, dt, steps, u0, v0)
    f.close()
    E = kin + pot
    assert (kin[0] == 0.0).all() and E[0] == pytest.approx(0.5 * np.einsum("ic,ij,jc->c", u0, c.A, u0), rel=1e-12)
    drift = float((np.abs(E - E[0]).max(axis=0) / E[0]).max())
    rise = 0.0
    for dlabel, dm, ds in ic.dampings(lam):
        f = _factor(c, ic.GAUSS, 2, dt, dm, ds)
        _, _, kin, pot = _wave(c, f, ic.GAUSS, dt, steps, u0, v0, dm, ds)
        f.close()
        Ed = kin + pot
        rise = max(rise, float(((Ed[1:] - Ed[:-1]) / Ed[:-1]).max()))
        assert (Ed[1:] <= Ed[:-1] * (1.0 + 1e-12)).all(), (name, dlabel, Ed)
        assert (Ed[-1] < Ed[0]).all()
    print("%s Gauss, %d steps at dt = 0.7 / omega_1: relative energy drift undamped %.3e; largest relative rise with damping %.3e"
          % (name, steps, drift, rise))
    assert drift <= 1e-8


@pytest.mark.parametrize("name", ic.CASES)
def test_radau_damps_the_highest_mode_in_one_step(so, name):
    torch, dev = _torch()
    c = ic.irk_case(so, name)
    lam = c.lam_h
    dt = 10.0 / lam[0]
    xn = c.X[:, -1]
    rng = np.random.default_rng(704)
    u0 = rng.uniform(-1.0, 1.0, (c.nrow, 2)) + xn[:, None] / np.abs(xn).max()
    start = xn @ (c.M @ u0)
    f = _factor(c, ic.RADAU, 1, dt)
    _, mass, cols = _ptrs(c)
    norms = [np.einsum("ic,ij,jc->c", u0, c.M, u0)]
    U = _dev(u0)
    sym = c.sym.data_ptr()
    for k in range(3):
        c.g.lod_irk_heat_steps(f, ic.RADAU, sym, cols, dt, 1, U.data_ptr(), n_rhs=2)
        norms.append(c.g.lod_inner(mass, cols, U.data_ptr(), U.data_ptr(), n_rhs=2))
        if k == 0:
            torch.cuda.synchronize()
            after = xn @ (c.M @ U.cpu().numpy())
    f.close()
    ratio = float(np.abs(after / start).max())
    print("%s Radau, dt = 10 / lambda_1: the highest mode falls to %.3e of its start in one step (|R| = %.3e); u^T M u %s"
          % (name, ratio, abs(ic.stability(ic.RADAU, -lam[-1] * dt)), " ".join("%.3e" % x for x in np.array(norms)[:, 0])))
    assert ratio < 1e-2
    assert (np.diff(np.array(norms), axis=0) <= 0.0).all(), norms


# ---- words

@pytest.mark.parametrize("name", ["rowmajor", "morton16"])
def test_irk_words(so, name):
    c = ic.irk_case(so, name)
    lam = c.lam_h
    u0, v0, loads = _data(c, 705)
    n, stage = 17, loads["stage"][:4]
    hdts, wdts = ic.heat_dts(lam), ic.wave_dts(lam)
    _, dm, ds = ic.dampings(lam)[2]
    for label, scheme in ic.SCHEMES:
        fh, fw = _factor(c, scheme, 1, hdts[1]), _factor(c, scheme, 2, wdts[0], dm, ds)
        dth, dtw = hdts[1], wdts[0]

        def heat(cols=slice(None), steps=2, ld=None, b=stage, u=u0, f=fh, member=0):
            return _heat(c, f, scheme, dth, steps, u[:, cols], None if b is None else b[:, :, cols], ld=ld, member=member)

        def wave(cols=slice(None), steps=2, ld=None, b=stage, u=u0, v=v0, f=fw, member=0):
            return _wave(c, f, scheme, dtw, steps, u[:, cols], v[:, cols], dm, ds, None if b is None else b[:, :, cols], ld=ld,
                         member=member)

        H = _bits(heat())
        Uw, Vw, kin, pot = wave()
        W = np.stack([_bits(Uw), _bits(Vw)])
        assert np.isfinite(Uw.cpu().numpy()).all() and np.isfinite(Vw.cpu().numpy()).all()
        # a repeated call
        assert np.array_equal(_bits(heat()), H)
        U2, V2, kin2, pot2 = wave()
        assert np.array_equal(np.stack([_bits(U2), _bits(V2)]), W)
        assert np.array_equal(kin2.view(np.uint64), kin.view(np.uint64)) and np.array_equal(pot2.view(np.uint64), pot.view(np.uint64))
        # n_steps = 2 is two calls with n_steps = 1, the second on the loads of the second step
        h1 = heat(steps=1, b=stage[:2])
        h2 = heat(steps=1, b=stage[2:], u=h1.cpu().numpy())
        assert np.array_equal(_bits(h2), H)
        Ua, Va, ka, pa = wave(steps=1, b=stage[:2])
        Ub, Vb, kb, pb = wave(steps=1, b=stage[2:], u=Ua.cpu().numpy(), v=Va.cpu().numpy())
        assert np.array_equal(np.stack([_bits(Ub), _bits(Vb)]), W)
        assert np.array_equal(np.concatenate([ka, kb[1:]]).view(np.uint64), kin.view(np.uint64))
        assert np.array_equal(np.concatenate([pa, pb[1:]]).view(np.uint64), pot.view(np.uint64))
        assert np.array_equal(ka[1].view(np.uint64), kb[0].view(np.uint64))
        # a column is its own n_rhs = 1 run
        for col in (0, 5, 16):
            assert np.array_equal(_bits(heat(cols=[col]))[:, 0], H[:, col])
            U1, V1, k1, p1 = wave(cols=[col])
            assert np.array_equal(_bits(U1)[:, 0], W[0][:, col]) and np.array_equal(_bits(V1)[:, 0], W[1][:, col])
            assert np.array_equal(k1[:, 0].view(np.uint64), kin[:, col].view(np.uint64))
            assert np.array_equal(p1[:, 0].view(np.uint64), pot[:, col].view(np.uint64))
        # permuted columns
        perm = np.random.default_rng(706).permutation(n)
        assert np.array_equal(_bits(heat(cols=perm)), H[:, perm])
        Up, Vp, kp, pp = wave(cols=perm)
        assert np.array_equal(_bits(Up), W[0][:, perm]) and np.array_equal(_bits(Vp), W[1][:, perm])
        assert np.array_equal(kp.view(np.uint64), kin[:, perm].view(np.uint64))
        # a padded leading dimension: the same words, the padding untouched
        ld = n + 6
        Hp = heat(ld=ld)
        assert np.array_equal(_bits(Hp)[:, :n], H) and bool(Hp[:, n:].isnan().all())
        Ul, Vl, _, _ = wave(ld=ld)
        assert np.array_equal(_bits(Ul)[:, :n], W[0]) and np.array_equal(_bits(Vl)[:, :n], W[1])
        assert bool(Ul[:, n:].isnan().all()) and bool(Vl[:, n:].isnan().all())
        # the energies do not touch the state: the same words with them off (no load)
        Un, Vn, _, _ = _wave(c, fw, scheme, dtw, 2, u0, v0, dm, ds, energies=False)
        Ue, Ve, _, _ = _wave(c, fw, scheme, dtw, 2, u0, v0, dm, ds)
        assert np.array_equal(_bits(Un), _bits(Ue)) and np.array_equal(_bits(Vn), _bits(Ve))
        # member 1 of a two-member factor (two dt) is the one-member factor
        f2h, f2w = _factor(c, scheme, 1, [hdts[0], dth]), _factor(c, scheme, 2, [wdts[1], dtw], dm, ds)
        assert np.array_equal(_bits(heat(f=f2h, member=1)), H)
        Um, Vm, km, pm = wave(f=f2w, member=1)
        assert np.array_equal(np.stack([_bits(Um), _bits(Vm)]), W) and np.array_equal(km.view(np.uint64), kin.view(np.uint64))
        assert not np.array_equal(_bits(heat(f=f2h, member=0)), H)
        for f in (fh, fw, f2h, f2w):
            f.close()


# ---- refusals

def test_irk_refusals_that_need_a_factor(so):
    import slod_amd
    torch, dev = _torch()
    c = ic.irk_case(so, "rowmajor")
    g = c.g
    sym, mass, cols = _ptrs(c)
    U0, V0, A0 = (_dev(np.ones((c.nrow, 1))) for _ in range(3))
    dt = ic.wave_dts(c.lam_h)[0]
    new = {"slod_lod_irk_heat_steps_direct": lambda f, **kw: g.lod_irk_heat_steps(f, "radau", sym, cols, dt, 1, U0.data_ptr(), **kw),
           "slod_lod_irk_wave_steps_direct": lambda f, **kw: g.lod_irk_wave_steps(f, "gauss", sym, mass, cols, dt, 1, U0.data_ptr(),
                                                                                V0.data_ptr(), **kw)}
    for real in (g.lod_factor(sym, cols), g.lod_factor_ldl(sym, cols)):
        for who, call in new.items():
            with pytest.raises(slod_amd.SlodError) as e:
                call(real)
            assert e.value.code == -1 and str(e.value).endswith(who + ": " + REFUSED), (who, str(e.value))
        real.close()
    z = _factor(c, ic.GAUSS, 2, [dt, 2.0 * dt])
    for who, call in new.items():
        for member in (-1, 2):
            with pytest.raises(slod_amd.SlodError) as e:
                call(z, member=member)
            assert e.value.code == -1 and str(e.value).endswith(who + ": member outside the factor"), str(e.value)
    # the real consumers go on refusing the complex factor
    text = "a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex"
    old = {"slod_lod_theta_steps_direct": lambda: g.lod_theta_steps_direct(z, sym, cols, dt, 0.5, 1, U0.data_ptr()),
           "slod_lod_newmark_steps_direct": lambda: g.lod_newmark_steps_direct(z, sym, mass, cols, dt, 1, U0.data_ptr(),
                                                                               V0.data_ptr(), A0.data_ptr())}
    for who, call in old.items():
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith(who + ": " + text), (who, str(e.value))
    # the factor of another handle
    other = slod_amd.Slod(n_cells=5, n_sub=3, oversampling=1, spacedim=1)
    for who in new:
        args = dict(slod_lod_irk_heat_steps_direct=(other.h, z.f, 0, 0, sym, cols, dt, 1, 1, U0.data_ptr(), 1, None, 1, 0),
                    slod_lod_irk_wave_steps_direct=(other.h, z.f, 0, 0, sym, mass, cols, dt, 0.0, 0.0, 1, 1, U0.data_ptr(), 1,
                                                    V0.data_ptr(), 1, None, 1, 0, None, None))[who]
        assert getattr(g.lib, who)(*args) == -1
        assert other.lib.slod_last_error(other.h).decode() == who + ": factor of another handle / row count"
    other.close()
    torch.cuda.synchronize()
    # no device work on a refusal: the states are untouched
    assert bool((U0 == 1.0).all()) and bool((V0 == 1.0).all()) and bool((A0 == 1.0).all())
    z.close()


# ---- the mirror and the driver

def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


FACTOR_LINE = r"^factor: n = (\d+), half bandwidth = (\d+), bytes = (\d+), pivots in \[(\S+), (\S+)\]$"
GROWTH_LINE = r"^factor: complex LDL\^T of the (\S+) step, growth = (\S+)$"


def test_driver_irk_matches_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --heat 4 DT --irk radau and --wave 4 DT --irk gauss (the driver's coefficient
    Alpha(1, 100, 3), srand(1); f = 1, constant in time; from u = 0, from rest) print the lines of --direct and the growth
    of the complex factor: every printed digit is that of the Python path."""
    from lod_cases import _build, _mass, _symmetrize
    torch, dev = _torch()
    steps, hdt, wdt = 4, 0.01, 0.005
    heat = _driver("--heat", str(steps), repr(hdt), "--irk", "radau")
    wave = _driver("--wave", str(steps), repr(wdt), "--irk", "gauss")
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    g = c.g
    c.mvalues, _ = _mass(c)
    c.sym = _symmetrize(c)
    sym, mass, cols = _ptrs(c)
    fld = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, fld.data_ptr())
    rhs = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
    g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, fld.data_ptr(), rhs.data_ptr())

    def factor_lines(out, f, scheme):
        m, gl = re.search(FACTOR_LINE, out, re.M), re.search(GROWTH_LINE, out, re.M)
        assert m and gl, out
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (f.info.n, f.info.half_bandwidth, f.info.bytes)
        assert (m.group(4), m.group(5)) == ("%.6e" % f.info.min_pivot, "%.6e" % f.info.max_pivot)
        assert (gl.group(1), gl.group(2)) == (scheme, "%.6e" % f.inertia(0).growth)

    # heat: the table of the final state against the elliptic solution
    assert re.findall(r"^heat step (\d+)$", heat, re.M) == ["1", "2", "3", "4"] and "iterations" not in heat
    f = _factor(c, ic.RADAU, 1, hdt)
    factor_lines(heat, f, "radau")
    uH, u = torch.zeros_like(rhs), torch.zeros_like(rhs)
    g.lod_solve(c.values.data_ptr(), cols, rhs.data_ptr(), uH.data_ptr(), 1e-13, 5000)
    g.lod_irk_heat_steps(f, "radau", sym, cols, hdt, steps, u.data_ptr(), d_load=rhs.data_ptr())
    f.close()
    fine_e, fine_t = torch.zeros_like(fld), torch.zeros_like(fld)
    g.lod_reconstruct(c.b.data_ptr(), c.stride, uH.data_ptr(), fine_e.data_ptr())
    g.lod_reconstruct(c.b.data_ptr(), c.stride, u.data_ptr(), fine_t.data_ptr())
    torch.cuda.synchronize()
    e, un = g.error_norms(fine_e.data_ptr(), fine_t.data_ptr()), g.error_norms(fine_e.data_ptr())
    table = heat.split("vs elliptic SLOD solution")[1]
    err = dict(re.findall(r"^  (\S+) +error = (\S+)", table, re.M))
    rel = dict(re.findall(r"^  (\S+) +error = \S+ +\(relative (\S+)\)", table, re.M))
    assert sorted(err) == ["H1", "L2", "Linfty", "energy"], heat
    for row, key in (("L2", "l2"), ("H1", "h1"), ("Linfty", "linf"), ("energy", "energy")):
        assert err[row] == "%.12e" % e[key], (row, err[row], e[key])
        assert rel[row] == "%.6e" % (e[key] / un[key]), (row, rel[row])
    # wave: energies and work per step, the norm of the final state
    f = _factor(c, ic.GAUSS, 2, wdt)
    factor_lines(wave, f, "gauss")
    lines = re.findall(r"^wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", wave, re.M)
    assert [m[0] for m in lines] == ["1", "2", "3", "4"], wave
    U, V = torch.zeros_like(rhs), torch.zeros_like(rhs)
    b = rhs.cpu().numpy()[:, 0]
    for k in range(steps):
        kin, pot = g.lod_irk_wave_steps(f, "gauss", sym, mass, cols, wdt, 1, U.data_ptr(), V.data_ptr(), d_load=rhs.data_ptr())
        work = 0.0
        for x, y in zip(U.cpu().numpy()[:, 0], b):                     # the driver's sum, in its order
            work += x * y
        assert lines[k][1:] == ("%.12e" % kin[1, 0], "%.12e" % pot[1, 0], "%.12e" % work), (k, lines[k])
    f.close()
    fine = torch.zeros_like(fld)
    g.lod_reconstruct(c.b.data_ptr(), c.stride, U.data_ptr(), fine.data_ptr())
    torch.cuda.synchronize()
    norm = re.search(r"^SLOD wave at T = \S+ L2 norm = (\S+)$", wave, re.M).group(1)
    assert norm == "%.12e" % g.error_norms(fine.data_ptr())["l2"]


# ---- the method: fourth order against the trapezoidal rule at the same step

def test_gauss_is_closer_than_the_trapezoidal_rule(so):
    """On the s2 pencil, from a smooth state (the five lowest modes) at dt = 0.5 / omega_1 per step over 8 steps: the
    distance to the same flow computed by Gauss with dt / 8 (whose error is 8^-4 of Gauss's own) is smaller for Gauss than
    for slod_lod_newmark_steps_direct with beta = 1/4.  The factor between them is printed, not asserted."""
    torch, dev = _torch()
    c = ic.irk_case(so, "s2")
    g, lam = c.g, c.lam_h
    sym, mass, cols = _ptrs(c)
    dt, steps = 0.5 / np.sqrt(lam[0]), 8
    u0 = c.X[:, :5] @ np.ones((5, 1))
    v0 = np.zeros_like(u0)
    f = _factor(c, ic.GAUSS, 2, [dt, dt / 8.0])
    Ug, _, _, _ = _wave(c, f, ic.GAUSS, dt, steps, u0, v0, member=0, energies=False)
    Uf, _, _, _ = _wave(c, f, ic.GAUSS, dt / 8.0, 8 * steps, u0, v0, member=1, energies=False)
    f.close()
    S = torch.full_like(c.sym, NAN)
    g.lod_matrix_combine(1.0, mass, 0.25 * dt * dt, sym, S.data_ptr())
    torch.cuda.synchronize()
    fM, fS = g.lod_factor(mass, cols), g.lod_factor(S.data_ptr(), cols)
    Ut, Vt, At = _dev(u0), _dev(v0), _dev(np.zeros_like(u0))
    g.lod_newmark_accel_direct(fM, sym, mass, cols, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr())
    g.lod_newmark_steps_direct(fS, sym, mass, cols, dt, steps, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr(), energies=False)
    torch.cuda.synchronize()
    fM.close()
    fS.close()
    fine = Uf.cpu().numpy()
    eg = float(np.abs(Ug.cpu().numpy() - fine).max() / np.abs(fine).max())
    et = float(np.abs(Ut.cpu().numpy() - fine).max() / np.abs(fine).max())
    print("s2, %d steps at dt = 0.5 / omega_1, distance to Gauss at dt / 8: Gauss %.3e, trapezoidal rule %.3e, factor %.1f"
          % (steps, eg, et, et / eg))
    assert eg < et
