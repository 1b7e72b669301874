"""GPU tests of slod_lod_inner_multi (x^T A y per column), slod_lod_newmark_accel (consistent initial acceleration) and
slod_lod_newmark_steps (Newmark-beta for M u'' + C u' + A u = b, C = damp_mass M + damp_stiff A) against dense numpy /
scipy on the same block rows, against closed forms of the scheme, against themselves (bits of a column depend on that
column only) and against the fine FEM wave equation run on the CPU.

Cases: step64 (nref 3, n_sub 2, l = 1, D100: 64 rows, 4 groups of 16), s2 (elasticity, 32 rows), rowmajor (25 rows:
the last group of 16 is partial), and for the bits of the bilinear form also s1 (16 rows: one group).  The stiffness is
always the device output of slod_lod_matrix_symmetrize.

Tolerances:
  inner product     0 against the numpy emulation of the summation order (64-bit words); 1e-12 relative against the
                    dense x^T A y (at most 64 x 98 products, each a few roundings) on a well-conditioned form
  accel, stepper    1e-8 of max |reference| with rel_tol = 1e-13, the tolerance of the theta tests
  closed form       1e-8 of max |x_j| after 12 steps (the dense model holds it to 2e-14)
  conservation      1e-8 relative over 10 steps (the dense model: 1e-15); decay: no increase beyond 1e-12 of the value
  driver            iterations equal, energies 1e-8 relative, |kinetic + potential - work| <= 1e-8 max potential
Time steps: for beta = 1/4, dt = 0.7 / omega_1 (about nine steps per period of the lowest mode, while the highest
modes are far beyond the explicit limit, so S mixes M and A); for beta = 0, dt = 1.8 / omega_max, inside the stability
limit 2 / omega_max; both frequencies from scipy.linalg.eigh of the dense pencil.  Damping: damp_mass = 0.1 omega_1,
damp_stiff = 0.1 / omega_max, modal damping ratios between 0.05 and 0.5.
The figures the tests print are recorded in DESIGN section 6, "Newmark stepper on the LOD space".
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_fields
from lod_cases import _apply, _bits, _build, _fem_reference, _mass, _mass_fine, _pencil, _symmetrize, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
NAN = float("nan")
TOL, MAXIT = 1e-13, 5000


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _omegas(c):
    """(omega_1, omega_max) of the dense pencil (c.lam from scipy.linalg.eigh(A, M))."""
    return math.sqrt(c.lam[0]), math.sqrt(c.lam[-1])


def _damping(c, damped):
    w1, wmax = _omegas(c)
    return (0.1 * w1, 0.1 / wmax) if damped else (0.0, 0.0)


def _padded(a, pad):
    """[nrow][n + pad] device array with NaN in the padding columns."""
    torch, dev = _torch()
    t = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=torch.float64, device=dev)
    t[:, :a.shape[1]] = _dev(a)
    return t


def _accel(c, U, V, A, n, load=None, ld_load=None, damp=(0.0, 0.0)):
    return c.g.lod_newmark_accel(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), U.data_ptr(), V.data_ptr(),
                                 A.data_ptr(), n_rhs=n, ld_u=U.shape[1], ld_v=V.shape[1], ld_a=A.shape[1],
                                 d_load=None if load is None else load.data_ptr(), ld_load=ld_load, damp_mass=damp[0],
                                 damp_stiff=damp[1], rel_tol=TOL, max_iterations=MAXIT)


def _steps(c, dt, beta, n_steps, U, V, A, n, load=None, ld_load=None, stride=0, damp=(0.0, 0.0), gamma=0.5, energies=True):
    return c.g.lod_newmark_steps(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), dt, n_steps, U.data_ptr(),
                                 V.data_ptr(), A.data_ptr(), beta=beta, gamma=gamma, n_rhs=n, ld_u=U.shape[1],
                                 ld_v=V.shape[1], ld_a=A.shape[1], d_load=None if load is None else load.data_ptr(),
                                 ld_load=ld_load, load_step_stride=stride, damp_mass=damp[0], damp_stiff=damp[1],
                                 rel_tol=TOL, max_iterations=MAXIT, energies=energies)


def _model_accel(c, u, v, b, damp):
    return np.linalg.solve(c.M, b - c.A @ (u + damp[1] * v) - damp[0] * (c.M @ v))


def _model_steps(c, dt, beta, gamma, n_steps, u, v, a, loads, damp):
    """The dense recursion; loads(k) = b^k.  Returns the final u, v, a and the energies of all levels."""
    C = damp[0] * c.M + damp[1] * c.A
    S = c.M + gamma * dt * C + beta * dt * dt * c.A
    kin, pot = [0.5 * np.sum(v * (c.M @ v), axis=0)], [0.5 * np.sum(u * (c.A @ u), axis=0)]
    for k in range(n_steps):
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        a = np.linalg.solve(S, loads(k + 1) - c.A @ ut - C @ vt)
        u = ut + beta * dt * dt * a
        v = vt + gamma * dt * a
        kin.append(0.5 * np.sum(v * (c.M @ v), axis=0))
        pot.append(0.5 * np.sum(u * (c.A @ u), axis=0))
    return u, v, a, np.array(kin), np.array(pot)


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


# ---- 1. the bilinear form

def _emulate_inner(x, Ay):
    """Elementwise product, sequential sums over groups of 16 rows (a short group is filled with zeros, as the kernel
    does), then over the groups in ascending order from 0."""
    prod = x * Ay
    nrow, n = prod.shape
    out = np.zeros(n)
    for g0 in range(0, nrow, 16):
        rows = np.zeros((16, n))
        rows[:min(16, nrow - g0)] = prod[g0:g0 + 16]
        part = rows[0].copy()
        for r in range(1, 16):
            part = part + rows[r]
        out = out + part
    return out


@pytest.mark.parametrize("name", ["s1", "s2", "rowmajor"])
def test_inner_product_bits_and_dense_value(so, name):
    torch, dev = _torch()
    c = _pencil(so, name)
    K = 65
    rng = np.random.default_rng(41)
    # y = x + r / 4: x^T A y is dominated by x^T A x > 0, so the form is well conditioned and a bound relative to its
    # value means something (for independent random x and y the value is the remainder of a cancellation)
    hx = rng.uniform(-1.0, 1.0, (c.nrow, K))
    X, Y = _dev(hx), _dev(hx + 0.25 * rng.uniform(-1.0, 1.0, (c.nrow, K)))
    for which, values, dense in (("A", c.sym, c.A), ("M", c.mvalues, c.M)):
        AY = _apply(c, values, Y, K).cpu().numpy()
        AX = _apply(c, values, X, K).cpu().numpy()
        ref_xy, ref_xx = _emulate_inner(X.cpu().numpy(), AY), _emulate_inner(X.cpu().numpy(), AX)
        wide = c.g.lod_inner(values.data_ptr(), c.cols.data_ptr(), X.data_ptr(), Y.data_ptr(), n_rhs=K)
        quad = c.g.lod_inner(values.data_ptr(), c.cols.data_ptr(), X.data_ptr(), X.data_ptr(), n_rhs=K)
        assert np.array_equal(wide.view(np.uint64), ref_xy.view(np.uint64)), which
        assert np.array_equal(quad.view(np.uint64), ref_xx.view(np.uint64)), which
        hx, hy = X.cpu().numpy(), Y.cpu().numpy()
        exact, exact_q = np.sum(hx * (dense @ hy), axis=0), np.sum(hx * (dense @ hx), axis=0)
        print("%s %s: max relative deviation from the dense x^T A y %.3e, x^T A x %.3e"
              % (name, which, (np.abs(wide - exact) / np.abs(exact)).max(), (np.abs(quad - exact_q) / np.abs(exact_q)).max()))
        assert (np.abs(wide - exact) <= 1e-12 * np.abs(exact)).all()
        assert (np.abs(quad - exact_q) <= 1e-12 * np.abs(exact_q)).all()
        for n in (1, 3, 65):
            Xn, Yn = X[:, :n].contiguous(), Y[:, :n].contiguous()
            out = c.g.lod_inner(values.data_ptr(), c.cols.data_ptr(), Xn.data_ptr(), Yn.data_ptr(), n_rhs=n)
            assert np.array_equal(out.view(np.uint64), ref_xy[:n].view(np.uint64)), (which, n)
        for k in (0, 2, 63, 64):                       # column k of the wide arrays as an n_rhs = 1 call, ld = 65
            out = c.g.lod_inner(values.data_ptr(), c.cols.data_ptr(), X.data_ptr() + 8 * k, Y.data_ptr() + 8 * k, n_rhs=1,
                                ld_x=K, ld_y=K)
            assert out.view(np.uint64)[0] == ref_xy.view(np.uint64)[k], (which, k)
        Xw, Yw = _padded(X.cpu().numpy(), 5), _padded(Y.cpu().numpy(), 7)
        out = c.g.lod_inner(values.data_ptr(), c.cols.data_ptr(), Xw.data_ptr(), Yw.data_ptr(), n_rhs=K, ld_x=K + 5, ld_y=K + 7)
        assert np.array_equal(out.view(np.uint64), ref_xy.view(np.uint64)), which
        perm = torch.from_numpy(np.random.default_rng(43).permutation(K)).to(dev)
        Xp, Yp = X[:, perm].contiguous(), Y[:, perm].contiguous()
        out = c.g.lod_inner(values.data_ptr(), c.cols.data_ptr(), Xp.data_ptr(), Yp.data_ptr(), n_rhs=K)
        assert np.array_equal(out.view(np.uint64), ref_xy[perm.cpu().numpy()].view(np.uint64)), which


def test_inner_product_walks_more_groups_than_blocks():
    """8192 rows are 512 groups of 16 rows, more than the 256 blocks of a launch: every block walks two groups.  The
    form needs no basis, so the matrix is synthetic: 9 random columns per row, the rest unused."""
    import slod_amd
    torch, dev = _torch()
    g = slod_amd.Slod(nref=6, n_sub=1, oversampling=1, spacedim=2)
    NP, cap, s, n = g.num_patches, g.lod_row_capacity(), 2, 3
    rng = np.random.default_rng(47)
    cols = np.full((NP, cap), 0xffffffff, dtype=np.uint32)
    cols[:, :9] = rng.integers(0, NP, (NP, 9))
    vals = rng.uniform(-1.0, 1.0, (NP, cap, s, s))
    vals[cols == 0xffffffff] = NAN                     # an unused slot is never multiplied in
    X, Y = rng.uniform(-1.0, 1.0, (NP * s, n)), rng.uniform(-1.0, 1.0, (NP * s, n))
    vt, ct, xt, yt = _dev(vals), torch.from_numpy(cols.view(np.int32)).to(dev), _dev(X), _dev(Y)
    AY = torch.zeros_like(yt)
    g.lod_apply(vt.data_ptr(), ct.data_ptr(), yt.data_ptr(), AY.data_ptr(), n_rhs=n)
    torch.cuda.synchronize()
    out = g.lod_inner(vt.data_ptr(), ct.data_ptr(), xt.data_ptr(), yt.data_ptr(), n_rhs=n)
    assert np.array_equal(out.view(np.uint64), _emulate_inner(X, AY.cpu().numpy()).view(np.uint64))


# ---- 2. initial acceleration

@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("name", ["step64", "s2", "rowmajor"])
def test_accel_matches_dense_solve(so, name, damped):
    torch, dev = _torch()
    c = _pencil(so, name)
    n, damp = 3, _damping(c, damped)
    rng = np.random.default_rng(53)
    u, v = rng.uniform(-1e-3, 1e-3, (c.nrow, n)), rng.uniform(-1e-2, 1e-2, (c.nrow, n))
    b = rng.uniform(-1.0, 1.0, (c.nrow, n)) * np.abs(c.M).max()
    u[:, 1] = v[:, 1] = b[:, 1] = 0.0                  # a zero column: a = 0, 0 iterations
    U, V, B = _padded(u, 2), _padded(v, 1), _padded(b, 3)
    A = torch.full((c.nrow, n + 4), NAN, dtype=torch.float64, device=dev)
    its, res = _accel(c, U, V, A, n, load=B, ld_load=n + 3, damp=damp)
    ref = _model_accel(c, u, v, b, damp)
    err = _rel(A[:, :n].cpu().numpy(), ref)
    print("%s damped %s: accel iterations %s, residuals %s, relative error %.3e" % (name, damped, its.tolist(), res.tolist(), err))
    assert err <= 1e-8
    assert its[1] == 0 and res[1] == 0.0 and its[0] > 0 and its[2] > 0 and (res <= TOL).all()
    assert np.array_equal(_bits(A[:, 1]), np.zeros(c.nrow, np.uint64))
    assert bool(torch.isnan(A[:, n:]).all()) and bool(torch.isnan(U[:, n:]).all())
    assert np.array_equal(U[:, :n].cpu().numpy(), u) and np.array_equal(V[:, :n].cpu().numpy(), v)   # inputs are read only
    # without a load
    its0, _ = _accel(c, U, V, A, n, damp=damp)
    assert _rel(A[:, :n].cpu().numpy(), _model_accel(c, u, v, np.zeros_like(b), damp)) <= 1e-8 and its0[1] == 0


# ---- 3. the dense recursion

def _level_loads(c, n_levels, n, seed):
    """[level][row][column] coarse loads of the size of the entries of M (a load is C^T f, an integral against phi)."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n_levels, c.nrow, n)) * np.abs(c.M).max()


@pytest.mark.parametrize("name,beta,loading,damped",
                         [(nm, beta, loading, False) for nm in ("step64", "s2", "rowmajor") for beta in (0.25, 0.0)
                          for loading in ("none", "constant", "distinct")]
                         + [(nm, 0.25, "distinct", True) for nm in ("step64", "s2", "rowmajor")])
def test_newmark_steps_match_dense_recursion(so, name, beta, loading, damped):
    torch, dev = _torch()
    c = _pencil(so, name)
    w1, wmax = _omegas(c)
    dt = 0.7 / w1 if beta > 0.0 else 1.8 / wmax
    n, steps, damp = 2, 3, _damping(c, damped)
    rng = np.random.default_rng(59)
    u0, v0 = rng.uniform(-1e-3, 1e-3, (c.nrow, n)), rng.uniform(-1e-3, 1e-3, (c.nrow, n)) * w1
    L = _level_loads(c, steps + 1, n, 61)
    if loading == "none":
        loads, Lt, stride = (lambda k: np.zeros((c.nrow, n))), None, 0
    elif loading == "constant":
        loads, Lt, stride = (lambda k: L[1]), _dev(L[1]), 0
    else:
        loads, Lt, stride = (lambda k: L[k]), _dev(L), c.nrow * n
    U, V = _dev(u0), _dev(v0)
    A = torch.full((c.nrow, n), NAN, dtype=torch.float64, device=dev)
    _accel(c, U, V, A, n, load=None if Lt is None else Lt, ld_load=n, damp=damp)       # b^0 sits at the base of the loads
    a0 = _model_accel(c, u0, v0, loads(0), damp)
    assert _rel(A.cpu().numpy(), a0) <= 1e-8
    its, res, kin, pot = _steps(c, dt, beta, steps, U, V, A, n, load=Lt, ld_load=n, stride=stride, damp=damp)
    ur, vr, ar, kr, pr = _model_steps(c, dt, beta, 0.5, steps, u0, v0, a0, loads, damp)
    errs = [_rel(U.cpu().numpy(), ur), _rel(V.cpu().numpy(), vr), _rel(A.cpu().numpy(), ar), _rel(kin, kr), _rel(pot, pr)]
    print("%s beta %.2f, load %s, damped %s, dt %.3e: iterations %s, worst residual %.2e, relative errors u %.3e v %.3e a %.3e "
          "kinetic %.3e potential %.3e" % (name, beta, loading, damped, dt, its.tolist(), res.max(), *errs))
    assert len(its) == steps and (its > 0).all() and (its < MAXIT).all() and (res <= TOL).all()
    assert kin.shape == pot.shape == (steps + 1, n)
    assert max(errs) <= 1e-8


# ---- 4. closed form per mode

@pytest.mark.parametrize("which,beta,wdt", [("lowest", 0.25, 0.7), ("highest", 0.0, 1.8)])
def test_newmark_single_mode_follows_closed_form(so, which, beta, wdt):
    """u^0 = x_j, v^0 = 0, no load, no damping: u^k = cos(k theta) x_j, cos theta = 1 - (w dt)^2 / (2 (1 + beta (w dt)^2))."""
    torch, dev = _torch()
    c = _pencil(so, "step64")
    j = 0 if which == "lowest" else c.nrow - 1
    w, x = math.sqrt(c.lam[j]), c.vec[:, j]
    dt, steps = wdt / w, 12
    theta = math.acos(1.0 - wdt * wdt / (2.0 * (1.0 + beta * wdt * wdt)))
    U, V = _dev(x.reshape(-1, 1)), _dev(np.zeros((c.nrow, 1)))
    A = torch.full((c.nrow, 1), NAN, dtype=torch.float64, device=dev)
    _accel(c, U, V, A, 1)
    assert _rel(A.cpu().numpy()[:, 0], -c.lam[j] * x) <= 1e-8
    worst = 0.0
    for k in range(1, steps + 1):
        its, res, _, _ = _steps(c, dt, beta, 1, U, V, A, 1)
        assert (res <= TOL).all()
        worst = max(worst, np.abs(U.cpu().numpy()[:, 0] - math.cos(k * theta) * x).max() / np.abs(x).max())
    print("%s mode, omega %.4f, omega dt %.1f, beta %.2f: max deviation from cos(k theta) x_j over %d steps %.3e"
          % (which, w, wdt, beta, steps, worst))
    assert worst <= 1e-8


# ---- 5. conservation and decay

def test_newmark_trapezoidal_conserves_energy_and_damping_dissipates(so):
    torch, dev = _torch()
    c = _pencil(so, "step64")
    w1, _ = _omegas(c)
    dt, steps = 0.7 / w1, 10
    u0 = np.random.default_rng(67).uniform(-1.0, 1.0, (c.nrow, 1))
    for damped in (False, True):
        damp = _damping(c, damped)
        U, V = _dev(u0), _dev(np.zeros_like(u0))
        A = torch.full((c.nrow, 1), NAN, dtype=torch.float64, device=dev)
        _accel(c, U, V, A, 1, damp=damp)
        its, res, kin, pot = _steps(c, dt, 0.25, steps, U, V, A, 1, damp=damp)
        E = (kin + pot)[:, 0]
        print("damped %s: kinetic + potential over %d trapezoidal steps: %s" % (damped, steps, ["%.9e" % e for e in E]))
        assert (res <= TOL).all() and E[0] > 0 and kin[0, 0] == 0.0
        assert E[0] == pytest.approx(0.5 * float(u0[:, 0] @ c.A @ u0[:, 0]), rel=1e-12)
        if not damped:
            assert np.abs(E - E[0]).max() <= 1e-8 * E[0]
        else:
            assert (E[1:] <= E[:-1] + 1e-12 * E[:-1]).all() and E[-1] < E[0]


# ---- 6. composition and column independence, as 64-bit words

@pytest.mark.parametrize("name,beta", [("step64", 0.25), ("step64", 0.0), ("rowmajor", 0.25)])
def test_newmark_steps_compose_and_columns_are_independent(so, name, beta):
    torch, dev = _torch()
    c = _pencil(so, name)
    w1, wmax = _omegas(c)
    dt = 0.7 / w1 if beta > 0.0 else 1.8 / wmax
    n, damp = 3, _damping(c, True)
    rng = np.random.default_rng(71)
    L = torch.full((3, c.nrow, n + 2), NAN, dtype=torch.float64, device=dev)            # [level][row][column]
    L[:, :, :n] = _dev(_level_loads(c, 3, n, 73))
    u0, v0 = rng.uniform(-1e-3, 1e-3, (c.nrow, n)), rng.uniform(-1e-3, 1e-3, (c.nrow, n)) * w1
    stride = c.nrow * (n + 2)

    def start():
        U, V = _padded(u0, 4), _padded(v0, 1)
        A = torch.full((c.nrow, n + 3), NAN, dtype=torch.float64, device=dev)
        _accel(c, U, V, A, n, load=L, ld_load=n + 2, damp=damp)
        return U, V, A

    U, V, A = start()
    its2, res2, kin2, pot2 = _steps(c, dt, beta, 2, U, V, A, n, load=L, ld_load=n + 2, stride=stride, damp=damp)
    for T in (U, V, A):                                                                # padding is never written
        assert bool(torch.isnan(T[:, n:]).all()) and bool(torch.isfinite(T[:, :n]).all())
    # two identical calls give identical words
    U1, V1, A1 = start()
    itsb, _, kinb, potb = _steps(c, dt, beta, 2, U1, V1, A1, n, load=L, ld_load=n + 2, stride=stride, damp=damp)
    for a, b in ((U, U1), (V, V1), (A, A1)):
        assert np.array_equal(_bits(a[:, :n]), _bits(b[:, :n]))
    assert itsb.tolist() == its2.tolist() and np.array_equal(kinb.view(np.uint64), kin2.view(np.uint64))
    assert np.array_equal(potb.view(np.uint64), pot2.view(np.uint64))
    # one call with n_steps = 2 equals two calls with n_steps = 1
    U1, V1, A1 = start()
    its1, kin1, pot1 = [], [], []
    for k in range(2):
        it, _, kk, pp = _steps(c, dt, beta, 1, U1, V1, A1, n, load=L[k], ld_load=n + 2, stride=stride, damp=damp)
        its1.append(int(it[0]))
        kin1 += [kk[0], kk[1]]
        pot1 += [pp[0], pp[1]]
    for a, b in ((U, U1), (V, V1), (A, A1)):
        assert np.array_equal(_bits(a[:, :n]), _bits(b[:, :n]))
    assert its1 == its2.tolist()
    for got, ref in ((kin1, kin2), (pot1, pot2)):
        assert np.array_equal(np.stack(got)[[0, 1, 2, 3]].view(np.uint64), ref[[0, 1, 1, 2]].view(np.uint64))
    # every column equals its own n_rhs = 1 run
    worst = []
    for col in range(n):
        u, v = _dev(u0[:, col:col + 1]), _dev(v0[:, col:col + 1])
        a = torch.full((c.nrow, 1), NAN, dtype=torch.float64, device=dev)
        Lc = L[:, :, col].contiguous()                                                 # [level][row], ld_load = 1
        _accel(c, u, v, a, 1, load=Lc, ld_load=1, damp=damp)
        it, _, kk, pp = _steps(c, dt, beta, 2, u, v, a, 1, load=Lc, ld_load=1, stride=c.nrow, damp=damp)
        for one, wide in ((u, U), (v, V), (a, A)):
            assert np.array_equal(_bits(one[:, 0]), _bits(wide[:, col])), col
        assert np.array_equal(kk[:, 0].view(np.uint64), kin2[:, col].copy().view(np.uint64)), col
        assert np.array_equal(pp[:, 0].view(np.uint64), pot2[:, col].copy().view(np.uint64)), col
        worst.append(it)
    assert np.array_equal(np.max(np.stack(worst), axis=0), its2)
    # without the energies the state is the same
    U1, V1, A1 = start()
    _, _, none_k, none_p = _steps(c, dt, beta, 2, U1, V1, A1, n, load=L, ld_load=n + 2, stride=stride, damp=damp, energies=False)
    assert none_k is None and none_p is None and np.array_equal(_bits(U1[:, :n]), _bits(U[:, :n]))


def test_newmark_zero_problem(so):
    """Zero state plus zero load gives zeros and 0 iterations."""
    torch, dev = _torch()
    c = _pencil(so, "step64")
    U, V, A = (torch.zeros(c.nrow, 2, dtype=torch.float64, device=dev) for _ in range(3))
    its, res = _accel(c, U, V, A, 2)
    assert its.tolist() == [0, 0] and res.tolist() == [0.0, 0.0]
    its, res, kin, pot = _steps(c, 0.01, 0.25, 2, U, V, A, 2)
    assert its.tolist() == [0, 0] and res.tolist() == [0.0, 0.0]
    for T in (U, V, A):
        assert np.array_equal(_bits(T), np.zeros((c.nrow, 2), np.uint64))
    assert not kin.any() and not pot.any()


# ---- 7. against the fine wave equation

def test_wave_converges_to_fine_wave_with_oversampling(so):
    """N = 8, n_sub = 2, D100, f = 1, from rest, trapezoidal rule, 8 steps up to half the period of the lowest fine mode:
    relative L2 error (slod_compute_error_norms) of the reconstructed LOD state against the same scheme with the same dt
    on the fine FEM matrices in scipy; strictly smaller for l = 2 than for l = 1."""
    import scipy.linalg as sl
    torch, dev = _torch()
    steps, beta, gamma = 8, 0.25, 0.5
    errs = []
    for ell in (1, 2):
        c = _build(so, dict(nref=3, n_sub=2, oversampling=ell, spacedim=1))
        g, NE = c.g, c.g.NE
        cfg = so.make_cfg(nref=3, n_sub=2, oversampling=ell, spacedim=1, stabilize=1)
        Ah, fh, idx = _fem_reference(NE, 1, make_fields(so, cfg, "D100"))
        Ah = Ah.toarray()
        Mh = _mass_fine(NE)[np.ix_(idx, idx)]
        w1 = math.sqrt(sl.eigh(Ah, Mh, eigvals_only=True)[0])
        dt = math.pi / w1 / steps
        Sh = Mh + beta * dt * dt * Ah
        u, v = np.zeros(len(idx)), np.zeros(len(idx))
        a = np.linalg.solve(Mh, fh)
        for _ in range(steps):
            ut, vt = u + dt * v + dt * dt * (0.5 - beta) * a, v + dt * (1.0 - gamma) * a
            a = np.linalg.solve(Sh, fh - Ah @ ut)
            u, v = ut + beta * dt * dt * a, vt + gamma * dt * a
        ref = np.zeros((NE + 1) ** 2)
        ref[idx] = u
        ref_t = _dev(ref)
        c.mvalues, _ = _mass(c)
        c.sym = _symmetrize(c)
        f = torch.zeros((NE + 1) ** 2, dtype=torch.float64, device=dev)
        g.fem_rhs(None, f.data_ptr())
        rhs = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
        g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, f.data_ptr(), rhs.data_ptr())
        U, V, A = (torch.zeros_like(rhs) for _ in range(3))
        _accel(c, U, V, A, 1, load=rhs, ld_load=1)
        its, res, kin, pot = _steps(c, dt, beta, steps, U, V, A, 1, load=rhs, ld_load=1)
        assert (res <= TOL).all()
        fine = torch.zeros_like(f)
        g.lod_reconstruct(c.b.data_ptr(), c.stride, U.data_ptr(), fine.data_ptr())
        torch.cuda.synchronize()
        errs.append(g.error_norms(fine.data_ptr(), ref_t.data_ptr())["l2"] / g.error_norms(ref_t.data_ptr())["l2"])
        print("wave, l = %d: omega_1,h %.4f, dt %.4e, iterations %s, relative L2 error at T = %.4f against FEM(h): %.4e"
              % (ell, w1, dt, its.tolist(), dt * steps, errs[-1]))
    assert errs[1] < errs[0], errs


# ---- 8. the driver

def test_driver_wave_matches_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --wave 4 0.005 (the driver's coefficient Alpha(1, 100, 3), srand(1); f = 1; trapezoidal
    rule from rest) prints per step the iterations, energies and the work u^T b; from rest under a constant load the
    trapezoidal rule keeps kinetic + potential - work = 0."""
    torch, dev = _torch()
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    steps, dt = 4, 0.005
    r = subprocess.run([BIN, "3", "4", "1", "1", "--wave", str(steps), str(dt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"^wave step (\d+): iterations = (\d+), relative residual = (\S+), kinetic = (\S+), potential = (\S+), "
                       r"work = (\S+)$", r.stdout, re.M)
    assert [int(m[0]) for m in lines] == list(range(1, steps + 1)), r.stdout
    its = [int(m[1]) for m in lines]
    resid, kin, pot, work = (np.array([float(m[i]) for m in lines]) for i in (2, 3, 4, 5))
    norm = float(re.search(r"^SLOD wave at T = \S+ L2 norm = (\S+)$", r.stdout, re.M).group(1))
    assert resid.max() <= TOL and (kin > 0).all() and (pot > 0).all()
    assert (np.abs(kin + pot - work) <= 1e-8 * pot.max()).all(), (kin, pot, work)
    # the Python path
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    g = c.g
    c.mvalues, _ = _mass(c)
    c.sym = _symmetrize(c)
    f = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, f.data_ptr())
    rhs = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
    g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, f.data_ptr(), rhs.data_ptr())
    U, V, A = (torch.zeros_like(rhs) for _ in range(3))
    _accel(c, U, V, A, 1, load=rhs, ld_load=1)
    pits, pres, pkin, ppot = _steps(c, dt, 0.25, steps, U, V, A, 1, load=rhs, ld_load=1)
    assert its == pits.tolist(), (its, pits)
    assert kin == pytest.approx(pkin[1:, 0], rel=1e-8) and pot == pytest.approx(ppot[1:, 0], rel=1e-8)
    assert work[-1] == pytest.approx(float((U * rhs).sum().item()), rel=1e-8)
    fine = torch.zeros_like(f)
    g.lod_reconstruct(c.b.data_ptr(), c.stride, U.data_ptr(), fine.data_ptr())
    torch.cuda.synchronize()
    assert norm == pytest.approx(g.error_norms(fine.data_ptr())["l2"], rel=1e-8)
