"""GPU tests of the direct solver on the LOD space (slod_lod_factor_create / _solve: banded Cholesky, factor once, solve
many) and of the time loops on a factor (slod_lod_theta_steps_direct, slod_lod_newmark_accel_direct,
slod_lod_newmark_steps_direct), against dense numpy / scipy on the same block rows, against the CG steppers, and against
themselves as 64-bit words.

Cases (n rows, half bandwidth b = s (w N + w) + s - 1, w = 2 l + 1):
  dense     nref 2, n_sub 2, l 1, s 1   n = 16,   b = 15   the band is the matrix, n is one tile
  rowmajor  5 cells, n_sub 3, l 1       n = 25,   b = 18   padding in n and in b, row-major ids
  s2        nref 3, n_sub 2, l 1, s 2   n = 128,  b = 55   elasticity
  morton16  nref 4, n_sub 2, l 1, s 1   n = 256,  b = 51   16 block columns, Morton ids: the permutation is not trivial
  c2geom    nref 5, n_sub 2, l 2, s 1   n = 1024, b = 165  no basis: a synthetic matrix on the pattern of slod_lod_pattern,
            symmetric off-diagonal entries uniform in [-1, 1], diagonal = absolute row sum + 1 (no decay across the band:
            a missing or misplaced term anywhere moves the solution by about 1e-3)
  wide4     nref 2, n_sub 1, l 2, s 1   n = 16,   b = 25   synthetic; 2 l + 1 > N: the band is wider than the matrix
            (bb = 2 > nb = 1, a single block row)
  wide5     5 cells, n_sub 1, l 2, s 2  n = 50,   b = 61   synthetic, s x s blocks; bb = 4 = nb
The first four carry three matrices each: sym(A_LOD), M_LOD and M + 0.01 A.

Bars:
  backward error  eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), residual in np.longdouble, at most
                  (3 (b + 1) + 1) (b + 1) 2^-53: Higham, Accuracy and Stability, Thm 10.4 for a Cholesky solve,
                  gamma_{3k+1} || |L| |L^T| || <= gamma_{3k+1} k ||A|| with inner products of length k <= b + 1
  forward error   1e-8 relative per column against numpy.linalg.solve, the project's bar for solves against dense
  bits            equality of 64-bit words
  steppers        1e-8 relative against the dense recursion and against the CG steppers at rel_tol = 1e-13
  conservation    1e-8 relative over 10 trapezoidal steps, the bar of the CG stepper's test
The implementation has one tile size (16) and keeps X in global memory for every geometry: there is no size-dependent
path and no knob, so no test runs "the other side" of one.
The figures the tests print are recorded in DESIGN section 6, "Direct solver on the LOD space".
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from lod_cases import _bits, _build, _mass, _pencil, _rows_to_dense, _symmetrize, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
NAN = float("nan")
U = 2.0 ** -53
CASES = ("dense", "rowmajor", "s2", "morton16", "c2geom", "wide4", "wide5")
_cases = {}


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _combine(c, alpha, a, beta, b):
    torch, dev = _torch()
    out = torch.full_like(a, NAN)
    c.g.lod_matrix_combine(alpha, a.data_ptr(), beta, b.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def _dense(c, values):
    return _rows_to_dense(c.g, values.cpu().numpy(), c.cols.cpu().numpy().view(np.uint32), c.s)


def _order(c):
    """perm[r] = the caller's row p s + d of factor index r = (cy N + cx) s + d."""
    g, s = c.g, c.s
    perm = np.zeros(c.nrow, dtype=np.int64)
    for p in range(g.num_patches):
        info = g.patch_layout(p)
        for d in range(s):
            perm[(info.cy * g.N + info.cx) * s + d] = p * s + d
    return perm


SYNTHETIC = {"c2geom": dict(nref=5, n_sub=2, oversampling=2, spacedim=1),
             "wide4": dict(nref=2, n_sub=1, oversampling=2, spacedim=1),
             "wide5": dict(n_cells=5, n_sub=1, oversampling=2, spacedim=2)}


def _synthetic(so, kw):
    """The handle alone, columns by slot from the pattern, values from a seeded default_rng: a symmetric matrix of
    s x s blocks on the pattern of slod_lod_pattern, off-diagonal entries uniform in [-1, 1], diagonal = absolute row
    sum + 1."""
    import slod_amd
    torch, dev = _torch()

    class C:
        pass
    c = C()
    c.g = g = slod_amd.Slod(**kw)
    c.s = s = kw["spacedim"]
    c.nrow = g.num_patches * s
    NP, cap, span = g.num_patches, g.lod_row_capacity(), 4 * kw["oversampling"] + 3
    centre = np.array([(g.patch_layout(p).cx, g.patch_layout(p).cy) for p in range(NP)])
    pid = {(int(x), int(y)): p for p, (x, y) in enumerate(centre)}
    cols = np.full((NP, cap), 0xffffffff, dtype=np.uint32)
    for p in range(NP):
        coupled = set(g.lod_pattern(p))
        for j in range(cap):
            q = pid.get((int(centre[p, 0]) + j % span - span // 2, int(centre[p, 1]) + j // span - span // 2))
            if q is not None and q in coupled:
                cols[p, j] = q
        assert (cols[p] != 0xffffffff).sum() == len(coupled)
    rng = np.random.default_rng(20251019)
    W = np.tril(rng.uniform(-1.0, 1.0, (c.nrow, c.nrow)), -1)
    mask = np.zeros((NP, NP), dtype=bool)
    rows = np.repeat(np.arange(NP), cap).reshape(NP, cap)
    used = cols != 0xffffffff
    mask[rows[used], cols[used].astype(np.int64)] = True
    assert np.array_equal(mask, mask.T)
    A = (W + W.T) * np.kron(mask, np.ones((s, s), dtype=bool))
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, np.abs(A).sum(axis=1) + 1.0)
    vals = np.zeros((NP, cap, s, s))
    vals[used] = A.reshape(NP, s, NP, s).transpose(0, 2, 1, 3)[rows[used], cols[used].astype(np.int64)]
    c.cols = torch.from_numpy(cols.view(np.int32).ravel()).to(dev)
    c.mats = [("synthetic", _dev(vals.ravel()), A)]
    assert np.array_equal(_dense(c, c.mats[0][1]), A)
    return c


def _case(so, name):
    """Handle, columns, and the matrices of a case as (label, device values, dense copy); built once."""
    if name not in _cases:
        if name in SYNTHETIC:
            c = _synthetic(so, SYNTHETIC[name])
        else:
            if name in ("dense", "rowmajor"):
                c = _pencil(so, "s1" if name == "dense" else "rowmajor")
            else:
                c = _build(so, dict(nref=3, n_sub=2, oversampling=1, spacedim=2) if name == "s2"
                           else dict(nref=4, n_sub=2, oversampling=1, spacedim=1))
                c.mvalues, _ = _mass(c)
                c.sym = _symmetrize(c)
                c.A, c.M = _dense(c, c.sym), _dense(c, c.mvalues)
                assert np.array_equal(c.A, c.A.T) and np.array_equal(c.M, c.M.T)
            mix = _combine(c, 1.0, c.mvalues, 0.01, c.sym)
            c.mats = [("sym(A)", c.sym, c.A), ("M", c.mvalues, c.M), ("M + 0.01 A", mix, _dense(c, mix))]
        c.perm = _order(c)
        w = 2 * c.g.cfg.oversampling + 1
        c.hbw = c.s * (w * c.g.N + w) + c.s - 1
        _cases[name] = c
    return _cases[name]


def _solve(f, B, n, ld_u=None, first=0):
    """Out of place into a NaN-filled [nrow][ld_u]; columns first .. first + n of B."""
    torch, dev = _torch()
    ld_u = n if ld_u is None else ld_u
    out = torch.full((B.shape[0], ld_u), NAN, dtype=torch.float64, device=dev)
    f.solve(B.data_ptr() + 8 * first, out.data_ptr(), n_rhs=n, ld_rhs=B.shape[1], ld_u=ld_u)
    torch.cuda.synchronize()
    return out


def _eta(A, x, b):
    """Normwise backward error per column, the residual in extended precision."""
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)
    an = np.abs(A).sum(axis=1).max()
    return np.array(np.abs(r).max(axis=0) / (an * np.abs(x).max(axis=0) + np.abs(b).max(axis=0)), dtype=np.float64)


def _bound(b):
    return (3 * (b + 1) + 1) * (b + 1) * U


# ---- 1, 2, 4. backward and forward error, info

@pytest.mark.parametrize("name", CASES)
def test_factor_solve_backward_and_forward_error(so, name):
    import scipy.linalg as sl
    c = _case(so, name)
    rng = np.random.default_rng(101)
    for label, values, A in c.mats:
        f = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
        info = f.info
        assert (info.n, info.half_bandwidth, info.block) == (c.nrow, c.hbw, 16), (info.n, info.half_bandwidth, info.block)
        assert info.bytes >= 8 * c.nrow * (c.hbw + 1) and info.min_pivot > 0.0
        d2 = np.diag(np.linalg.cholesky(A[np.ix_(c.perm, c.perm)])) ** 2
        assert info.min_pivot == pytest.approx(d2.min(), rel=1e-10) and info.max_pivot == pytest.approx(d2.max(), rel=1e-10)
        cho = sl.cho_factor(A)
        worst, worst_ref, worst_fwd = 0.0, 0.0, 0.0
        for n in (1, 3, 16, 17, 65):
            hb = rng.uniform(-1.0, 1.0, (c.nrow, n))
            x = _solve(f, _dev(hb), n).cpu().numpy()
            assert np.isfinite(x).all()
            eta, ref = _eta(A, x, hb), np.linalg.solve(A, hb)
            fwd = np.abs(x - ref).max(axis=0) / np.abs(ref).max(axis=0)
            worst, worst_fwd = max(worst, eta.max()), max(worst_fwd, fwd.max())
            worst_ref = max(worst_ref, _eta(A, sl.cho_solve(cho, hb), hb).max())
            assert (eta <= _bound(c.hbw)).all(), (label, n, eta.max(), _bound(c.hbw))
            assert (fwd <= 1e-8).all(), (label, n, fwd.max())
        print("%s %s: n %d, b %d, bytes %d, pivots [%.3e, %.3e]; backward error %.3e (bound %.3e, scipy cho_solve %.3e), "
              "forward error %.3e" % (name, label, info.n, info.half_bandwidth, info.bytes, info.min_pivot, info.max_pivot,
                                      worst, _bound(c.hbw), worst_ref, worst_fwd))
        f.close()


# ---- 3, 6. bits

@pytest.mark.parametrize("name", ["rowmajor", "morton16"])
def test_factor_solve_bits(so, name):
    torch, dev = _torch()
    c = _case(so, name)
    label, values, A = c.mats[2]
    f = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
    K = 65
    hb = np.random.default_rng(103).uniform(-1.0, 1.0, (c.nrow, K))
    B = _dev(hb)
    wide = _solve(f, B, K)
    ref = _bits(wide)
    assert (_eta(A, wide.cpu().numpy(), hb) <= _bound(c.hbw)).all()
    # a repeated solve
    assert np.array_equal(_bits(_solve(f, B, K)), ref)
    # a column as its own n_rhs = 1 run, ld = K
    for k in (0, 2, 15, 16, 63, 64):
        one = _solve(f, B, 1, first=k)
        assert np.array_equal(_bits(one[:, 0]), ref[:, k]), k
    # permuted columns
    perm = np.random.default_rng(107).permutation(K)
    got = _solve(f, B[:, torch.from_numpy(perm).to(dev)].contiguous(), K)
    assert np.array_equal(_bits(got), ref[:, perm])
    # padded ld_rhs / ld_u, NaN padding left untouched
    Bw = torch.full((c.nrow, K + 5), NAN, dtype=torch.float64, device=dev)
    Bw[:, :K] = B
    got = _solve(f, Bw, K, ld_u=K + 7)
    assert np.array_equal(_bits(got[:, :K]), ref) and bool(torch.isnan(got[:, K:]).all()) and bool(torch.isnan(Bw[:, K:]).all())
    # a column sub-range of a wider array, both sides
    Uw = torch.full((c.nrow, K), NAN, dtype=torch.float64, device=dev)
    f.solve(B.data_ptr() + 8 * 5, Uw.data_ptr() + 8 * 7, n_rhs=20, ld_rhs=K, ld_u=K)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Uw[:, 7:27]), ref[:, 5:25])
    assert bool(torch.isnan(Uw[:, :7]).all()) and bool(torch.isnan(Uw[:, 27:]).all())
    # in place
    for n in (1, 17, K):
        X = B[:, :n].clone()
        f.solve(X.data_ptr(), X.data_ptr(), n_rhs=n)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(X), ref[:, :n]), n
    # a second factor of the same matrix
    f2 = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
    assert np.array_equal(_bits(_solve(f2, B, K)), ref)
    assert np.array([f.info.min_pivot, f.info.max_pivot]).tobytes() == np.array([f2.info.min_pivot, f2.info.max_pivot]).tobytes()
    # a zero right-hand side: exact zeros of either sign
    Z = _solve(f, torch.zeros(c.nrow, 3, dtype=torch.float64, device=dev), 3).cpu().numpy()
    assert not np.isnan(Z).any() and (Z == 0.0).all()
    # the argument checks that need a factor
    lib = c.g.lib
    assert lib.slod_lod_factor_solve(f.f, None, 1, 1, B.data_ptr(), 1, None) == -1
    assert lib.slod_lod_factor_solve(f.f, B.data_ptr(), K, 0, wide.data_ptr(), K, None) == -1
    assert lib.slod_lod_factor_solve(f.f, B.data_ptr(), K - 1, K, wide.data_ptr(), K, None) == -1
    assert "slod_lod_factor_solve" in lib.slod_last_error(c.g.h).decode()
    f2.close()
    f.close()


# ---- 5. not positive definite

def test_factor_refuses_indefinite_and_nan(so):
    import ctypes as C
    import slod_amd
    torch, dev = _torch()
    c = _case(so, "morton16")
    _spectrum(c)                                       # scipy.linalg.eigh of the dense pencil
    assert c.lam[0] < 1000.0 < c.lam[-1], (c.lam[0], c.lam[-1])
    shifted = _combine(c, 1.0, c.sym, -1000.0, c.mvalues)
    holed = c.mats[2][1].clone()
    cap = c.g.lod_row_capacity()
    hc = c.cols.cpu().numpy().view(np.uint32).reshape(-1, cap)
    r = int(c.perm[c.nrow // 2])                       # a row in the middle of the band, s = 1: row = patch
    below = [j for j in range(cap) if hc[r, j] != 0xffffffff and list(c.perm).index(int(hc[r, j])) < c.nrow // 2]
    holed[r * cap + below[0]] = NAN                    # an entry of the lower triangle in factor order
    for what, values in (("indefinite", shifted), ("NaN", holed)):
        out = C.c_void_p(1)
        rc = c.g.lib.slod_lod_factor_create(c.g.h, values.data_ptr(), c.cols.data_ptr(), C.byref(out))
        msg = c.g.lib.slod_last_error(c.g.h).decode()
        print("%s: %d, %s" % (what, rc, msg))
        assert rc == -5 and out.value is None and "slod_lod_factor_create" in msg and re.search(r"pivot \d+", msg)
        with pytest.raises(slod_amd.SlodError) as e:
            c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
        assert e.value.code == -5
    label, values, A = c.mats[2]
    f = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
    hb = np.random.default_rng(109).uniform(-1.0, 1.0, (c.nrow, 3))
    assert (_eta(A, _solve(f, _dev(hb), 3).cpu().numpy(), hb) <= _bound(c.hbw)).all()
    f.close()


# ---- 7. theta stepper on a factor

def _theta_model(c, dt, theta, n_steps, u, loads):
    S = c.M + theta * dt * c.A
    for k in range(n_steps):
        g = theta * loads(k + 1) + (1.0 - theta) * loads(k) - c.A @ u
        u = u + np.linalg.solve(S, dt * g)
    return u


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", ["morton16", "s2"])
def test_theta_steps_on_a_factor(so, name):
    torch, dev = _torch()
    c = _case(so, name)
    g, dt, steps = c.g, 0.01, 3
    sym, mass, cols = c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr()
    rng = np.random.default_rng(113)
    worst_dense, worst_cg = 0.0, 0.0
    for theta in (1.0, 0.5):
        S = _combine(c, 1.0, c.mvalues, theta * dt, c.sym)
        f = g.lod_factor(S.data_ptr(), cols)
        for n in (1, 3):
            u0 = rng.uniform(-1.0, 1.0, (c.nrow, n))
            L = rng.uniform(-1.0, 1.0, (steps + 1, c.nrow, n)) * np.abs(c.M).max()
            Lt = _dev(L)
            for loading in ("none", "constant", "distinct"):
                load, stride, loads = {"none": (None, 0, lambda k: np.zeros((c.nrow, n))),
                                       "constant": (Lt[1].data_ptr(), 0, lambda k: L[1]),
                                       "distinct": (Lt.data_ptr(), c.nrow * n, lambda k: L[k])}[loading]
                Ud, Uc = _dev(u0), _dev(u0)
                g.lod_theta_steps_direct(f, sym, cols, dt, theta, steps, Ud.data_ptr(), n_rhs=n, d_load=load,
                                         load_step_stride=stride)               # one factor, every call of this theta
                g.lod_theta_steps(sym, mass, cols, dt, theta, steps, Uc.data_ptr(), n_rhs=n, d_load=load,
                                  load_step_stride=stride, rel_tol=1e-13, max_iterations=5000)
                e_dense = _rel(Ud.cpu().numpy(), _theta_model(c, dt, theta, steps, u0, loads))
                e_cg = _rel(Ud.cpu().numpy(), Uc.cpu().numpy())
                worst_dense, worst_cg = max(worst_dense, e_dense), max(worst_cg, e_cg)
                assert e_dense <= 1e-8 and e_cg <= 1e-8, (theta, n, loading, e_dense, e_cg)
        # n_steps = 2 equals 2 x n_steps = 1, and a column equals its own run, as words; padded ld
        n = 3
        u0 = rng.uniform(-1.0, 1.0, (c.nrow, n))
        L = torch.full((3, c.nrow, n + 2), NAN, dtype=torch.float64, device=dev)
        L[:, :, :n] = _dev(rng.uniform(-1.0, 1.0, (3, c.nrow, n)) * np.abs(c.M).max())
        stride = c.nrow * (n + 2)

        def start():
            t = torch.full((c.nrow, n + 4), NAN, dtype=torch.float64, device=dev)
            t[:, :n] = _dev(u0)
            return t
        U2 = start()
        g.lod_theta_steps_direct(f, sym, cols, dt, theta, 2, U2.data_ptr(), n_rhs=n, ld_u=n + 4, d_load=L.data_ptr(),
                                 ld_load=n + 2, load_step_stride=stride)
        assert bool(torch.isnan(U2[:, n:]).all()) and bool(torch.isfinite(U2[:, :n]).all())
        U1 = start()
        for k in range(2):
            g.lod_theta_steps_direct(f, sym, cols, dt, theta, 1, U1.data_ptr(), n_rhs=n, ld_u=n + 4, d_load=L[k].data_ptr(),
                                     ld_load=n + 2, load_step_stride=stride)
        assert np.array_equal(_bits(U1[:, :n]), _bits(U2[:, :n]))
        for col in range(n):
            u = _dev(u0[:, col:col + 1])
            Lc = L[:, :, col].contiguous()
            g.lod_theta_steps_direct(f, sym, cols, dt, theta, 2, u.data_ptr(), d_load=Lc.data_ptr(), load_step_stride=c.nrow)
            assert np.array_equal(_bits(u[:, 0]), _bits(U2[:, col])), col
        f.close()
    print("%s: theta steps on a factor, worst relative deviation from the dense recursion %.3e, from the CG stepper %.3e"
          % (name, worst_dense, worst_cg))


def test_stepper_refuses_the_factor_of_another_handle(so):
    import slod_amd
    c, other = _case(so, "morton16"), _case(so, "dense")
    f = other.g.lod_factor(other.mvalues.data_ptr(), other.cols.data_ptr())
    torch, dev = _torch()
    u = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
    for call in (lambda: c.g.lod_theta_steps_direct(f, c.sym.data_ptr(), c.cols.data_ptr(), 0.01, 1.0, 1, u.data_ptr()),
                 lambda: c.g.lod_newmark_accel_direct(f, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), u.data_ptr(),
                                                      u.data_ptr(), u.data_ptr()),
                 lambda: c.g.lod_newmark_steps_direct(f, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), 0.01, 1,
                                                      u.data_ptr(), u.data_ptr(), u.data_ptr())):
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and "factor of another handle" in str(e.value)
    f.close()


# ---- 8. Newmark on a factor

def _spectrum(c):
    import scipy.linalg as sl
    if not hasattr(c, "lam"):
        c.lam = sl.eigh(c.A, c.M, eigvals_only=True)
    return math.sqrt(c.lam[0]), math.sqrt(c.lam[-1])


def _nm_model(c, dt, beta, gamma, n_steps, u, v, a, loads, damp):
    Cd = damp[0] * c.M + damp[1] * c.A
    S = c.M + gamma * dt * Cd + beta * dt * dt * c.A
    kin, pot = [0.5 * np.sum(v * (c.M @ v), axis=0)], [0.5 * np.sum(u * (c.A @ u), axis=0)]
    for k in range(n_steps):
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        a = np.linalg.solve(S, loads(k + 1) - c.A @ ut - Cd @ vt)
        u, v = ut + beta * dt * dt * a, vt + gamma * dt * a
        kin.append(0.5 * np.sum(v * (c.M @ v), axis=0))
        pot.append(0.5 * np.sum(u * (c.A @ u), axis=0))
    return u, v, a, np.array(kin), np.array(pot)


def _nm_factor(c, dt, beta, gamma, damp):
    S = _combine(c, 1.0 + gamma * dt * damp[0], c.mvalues, beta * dt * dt + gamma * dt * damp[1], c.sym)
    return c.g.lod_factor(S.data_ptr(), c.cols.data_ptr())


@pytest.mark.parametrize("beta,damped", [(0.25, False), (0.25, True), (0.0, False), (0.0, True)])
@pytest.mark.parametrize("name", ["morton16", "s2"])
def test_newmark_on_a_factor_matches_dense_recursion(so, name, beta, damped):
    torch, dev = _torch()
    c = _case(so, name)
    g = c.g
    w1, wmax = _spectrum(c)
    dt = 0.7 / w1 if beta > 0.0 else 1.8 / wmax
    damp = (0.1 * w1, 0.1 / wmax) if damped else (0.0, 0.0)
    n, steps, gamma = 2, 3, 0.5
    sym, mass, cols = c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr()
    rng = np.random.default_rng(127)
    u0, v0 = rng.uniform(-1e-3, 1e-3, (c.nrow, n)), rng.uniform(-1e-3, 1e-3, (c.nrow, n)) * w1
    L = rng.uniform(-1.0, 1.0, (steps + 1, c.nrow, n)) * np.abs(c.M).max()
    Lt = _dev(L)
    fM = g.lod_factor(mass, cols)
    fS = _nm_factor(c, dt, beta, gamma, damp)
    Ut, Vt = _dev(u0), _dev(v0)
    At = torch.full((c.nrow, n), NAN, dtype=torch.float64, device=dev)
    g.lod_newmark_accel_direct(fM, sym, mass, cols, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr(), n_rhs=n, d_load=Lt.data_ptr(),
                               damp_mass=damp[0], damp_stiff=damp[1])
    a0 = np.linalg.solve(c.M, L[0] - c.A @ (u0 + damp[1] * v0) - damp[0] * (c.M @ v0))
    e_a = _rel(At.cpu().numpy(), a0)
    assert e_a <= 1e-8, e_a

    def run(n_steps, Ut, Vt, At, first=0):
        return g.lod_newmark_steps_direct(fS, sym, mass, cols, dt, n_steps, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr(), beta=beta,
                                          gamma=gamma, n_rhs=n, d_load=Lt[first].data_ptr(), load_step_stride=c.nrow * n,
                                          damp_mass=damp[0], damp_stiff=damp[1])
    state = [t.clone() for t in (Ut, Vt, At)]
    kin, pot = run(steps, Ut, Vt, At)
    ur, vr, ar, kr, pr = _nm_model(c, dt, beta, gamma, steps, u0, v0, a0, lambda k: L[k], damp)
    errs = [_rel(Ut.cpu().numpy(), ur), _rel(Vt.cpu().numpy(), vr), _rel(At.cpu().numpy(), ar), _rel(kin, kr), _rel(pot, pr)]
    print("%s beta %.2f damped %s dt %.3e: relative errors accel %.3e, u %.3e v %.3e a %.3e kinetic %.3e potential %.3e"
          % (name, beta, damped, dt, e_a, *errs))
    assert kin.shape == pot.shape == (steps + 1, n) and max(errs) <= 1e-8
    # n_steps = 2 equals 2 x n_steps = 1, as words
    two = [t.clone() for t in state]
    k2, p2 = run(2, *two)
    one = [t.clone() for t in state]
    ka, pa = run(1, *one)
    kb, pb = run(1, *one, first=1)
    for a, b in zip(one, two):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(np.stack([ka[0], ka[1], kb[1]]).view(np.uint64), k2.view(np.uint64))
    assert np.array_equal(np.stack([pa[0], pa[1], pb[1]]).view(np.uint64), p2.view(np.uint64))
    assert np.array_equal(ka[1].view(np.uint64), kb[0].view(np.uint64))
    fM.close()
    fS.close()


def test_newmark_on_a_factor_conserves_energy(so):
    torch, dev = _torch()
    c = _case(so, "morton16")
    g = c.g
    w1, _ = _spectrum(c)
    dt, steps = 0.7 / w1, 10
    sym, mass, cols = c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr()
    u0 = np.random.default_rng(131).uniform(-1.0, 1.0, (c.nrow, 1))
    fM, fS = g.lod_factor(mass, cols), _nm_factor(c, dt, 0.25, 0.5, (0.0, 0.0))
    drift = {}
    for how in ("factor", "cg"):
        Ut, Vt = _dev(u0), _dev(np.zeros_like(u0))
        At = torch.full((c.nrow, 1), NAN, dtype=torch.float64, device=dev)
        if how == "factor":
            g.lod_newmark_accel_direct(fM, sym, mass, cols, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr())
            kin, pot = g.lod_newmark_steps_direct(fS, sym, mass, cols, dt, steps, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr())
        else:
            g.lod_newmark_accel(sym, mass, cols, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr(), rel_tol=1e-13, max_iterations=5000)
            _, _, kin, pot = g.lod_newmark_steps(sym, mass, cols, dt, steps, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr(),
                                                 rel_tol=1e-13, max_iterations=5000)
        E = (kin + pot)[:, 0]
        drift[how] = np.abs(E - E[0]).max() / E[0]
        assert E[0] == pytest.approx(0.5 * float(u0[:, 0] @ c.A @ u0[:, 0]), rel=1e-12) and kin[0, 0] == 0.0
    print("trapezoidal rule, %d steps, relative energy drift: on the factor %.3e, CG stepper at rel_tol 1e-13 %.3e"
          % (steps, drift["factor"], drift["cg"]))
    assert drift["factor"] <= 1e-8
    fM.close()
    fS.close()


# ---- 9. the driver

def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


FACTOR_LINE = r"^factor: n = (\d+), half bandwidth = (\d+), bytes = (\d+), pivots in \[(\S+), (\S+)\]$"


def test_driver_heat_direct():
    cg, direct = _driver("--heat", "4", "0.01"), _driver("--heat", "4", "0.01", "--direct")
    m = re.search(FACTOR_LINE, direct, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (64, 27) and float(m.group(4)) > 0.0, direct
    assert re.findall(r"^heat step (\d+)$", direct, re.M) == ["1", "2", "3", "4"] and "iterations" not in direct
    tables = []
    for out in (cg, direct):
        table = out.split("vs elliptic SLOD solution")[1]
        tables.append({k: float(v) for k, v in re.findall(r"^  (\S+) +error = (\S+)", table, re.M)})
    assert sorted(tables[0]) == sorted(tables[1]) == ["H1", "L2", "Linfty", "energy"]
    for k in tables[0]:
        print("heat %s distance: CG %.12e, direct %.12e" % (k, tables[0][k], tables[1][k]))
    for k in tables[0]:
        assert tables[1][k] == pytest.approx(tables[0][k], rel=1e-8), k


def test_driver_wave_direct():
    cg, direct = _driver("--wave", "4", "0.005"), _driver("--wave", "4", "0.005", "--direct")
    m = re.search(FACTOR_LINE, direct, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (64, 27) and float(m.group(4)) > 0.0, direct
    old = re.findall(r"^wave step (\d+): iterations = \d+, relative residual = \S+, kinetic = (\S+), potential = (\S+), work = (\S+)$",
                     cg, re.M)
    new = re.findall(r"^wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", direct, re.M)
    assert [m[0] for m in new] == [m[0] for m in old] == ["1", "2", "3", "4"], direct
    for a, b in zip(old, new):
        print("wave step %s: CG %s, direct %s" % (a[0], a[1:], b[1:]))
    for a, b in zip(old, new):
        for x, y in zip(a[1:], b[1:]):
            assert float(y) == pytest.approx(float(x), rel=1e-8)
    norm = [float(re.search(r"^SLOD wave at T = \S+ L2 norm = (\S+)$", out, re.M).group(1)) for out in (cg, direct)]
    assert norm[1] == pytest.approx(norm[0], rel=1e-8)
