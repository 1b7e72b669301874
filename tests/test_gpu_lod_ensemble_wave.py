"""Newmark time stepping on a coefficient ensemble on the GPU: the bilinear form, the consistent initial acceleration
and the stepper with a matrix, a factor and a column per member (slod_lod_inner_ensemble,
slod_lod_newmark_accel_ensemble_direct, slod_lod_newmark_steps_ensemble_direct).  Every comparison is one of 64-bit words
against the single-problem call (slod_lod_inner_multi, slod_lod_newmark_accel_direct, slod_lod_newmark_steps_direct with
n_rhs = 1) on the de-interleaved member unless it says otherwise.

Configurations (those of test_gpu_lod_ensemble_direct.py, built the same way: one handle with n_problems = 3, members
const / D100 / D1e4 of make_fields, one plan over all 3 * num_patches gids):
  base      nref 3, n_sub 2, l 1, s 1   64 rows
  s2        nref 3, n_sub 2, l 1, s 2   128 rows, elasticity
  rowmajor  5 cells, n_sub 3, l 1       25 rows, row-major ids
K = 65 (base only) takes the scaled copies (1 + k/64) member[k mod 3] of A and of M alike (the pencil of a copy is that
of its member) and crosses a wave of 64 members and the 64-column chunk of the tiling.

Time steps, as in test_gpu_lod_wave.py, from the dense pencils (scipy.linalg.eigh) of the three members: for beta = 1/4
dt = 0.7 / max_k omega_1(k); for beta = 0 dt = 1.8 / max_k omega_max(k), so that the stiffest member sets the step and
every member stays inside 2 / omega_max.  Damped: damp_mass = 0.3, damp_stiff = 1e-3; beta = 0 runs undamped only.

Bars that are not equality of words (those of test_gpu_lod_wave.py and test_gpu_lod_ensemble_direct.py):
  accel, stepper   1e-8 of max |reference| per member against the dense numpy recursion
  conservation     1e-8 relative over 10 trapezoidal steps without load and damping, per member
  decay            with damping no increase beyond 1e-12 of the value, and a lower end
  driver           |kinetic + potential - work| <= 1e-8 max potential per member
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_fields
from lod_cases import NAN, _bits, _lod_matrix, _rows_to_dense, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
DISTS = ("const", "D100", "D1e4")
CONFIGS = {"base": dict(nref=3, n_sub=2, oversampling=1, spacedim=1),
           "s2": dict(nref=3, n_sub=2, oversampling=1, spacedim=2),
           "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1)}
ROWS = {"base": 64, "s2": 128, "rowmajor": 25}
NAMES = sorted(CONFIGS)
CASES = [(name, 3) for name in NAMES] + [("base", 65)]
DAMPED = (0.3, 1e-3)
_cache = {}


class _Ens:
    pass


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _padded(a, pad):
    """[rows][n + pad] device array with NaN in the padding columns."""
    t = _nan(a.shape[0], a.shape[1] + pad)
    t[:, :a.shape[1]] = _dev(a)
    return t


def _case(so, name):
    """Handle, ensemble slab, and per member the single-problem A, sym(A), M and load vector (f = 1), the dense pencils
    and their extreme frequencies; built once and left unchanged."""
    if name in _cache:
        return _cache[name]
    import scipy.linalg as sl
    import slod_amd
    torch, dev = _torch()
    kw = CONFIGS[name]
    c = _Ens()
    c.s, c.K = kw["spacedim"], len(DISTS)
    cfg = so.make_cfg(stabilize=1, **kw)
    g = c.g = slod_amd.Slod(nref=kw.get("nref", 0), n_sub=kw["n_sub"], oversampling=kw["oversampling"], spacedim=c.s,
                            n_cells=kw.get("n_cells", 0), n_problems=c.K)
    for k, dist in enumerate(DISTS):
        for f, a in enumerate(make_fields(so, cfg, dist)):
            g.set_coefficient(f, a, problem=k)
    NP = c.NP = g.num_patches
    plan = g.plan(np.arange(c.K * NP, dtype=np.uint32))              # one plan over all members
    c.stride = plan.stride
    c.mstride = NP * c.stride
    c.b = torch.zeros(c.K * c.mstride, dtype=torch.float64, device=dev)
    c.q = torch.zeros_like(c.b)
    plan.execute(c.b.data_ptr(), c.q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    c.nrow, c.cap, c.field = NP * c.s, g.lod_row_capacity(), (g.NE + 1) ** 2 * c.s
    c.nval = NP * c.cap * c.s * c.s
    assert c.nrow == ROWS[name]
    c.slab = [(c.b[k * c.mstride:(k + 1) * c.mstride], c.q[k * c.mstride:(k + 1) * c.mstride]) for k in range(c.K)]
    c.values, c.cols = [], None
    for bk, qk in c.slab:
        v, cols = _lod_matrix(g, bk, qk, c.stride, c.s)
        c.values.append(v)
        assert c.cols is None or torch.equal(c.cols, cols)
        c.cols = cols
    c.hcols = c.cols.cpu().numpy().view(np.uint32)
    c.sym, c.mass = [], []
    for k in range(c.K):
        out = _nan(c.nval)
        g.lod_matrix_symmetrize(c.values[k].data_ptr(), c.cols.data_ptr(), out.data_ptr())
        c.sym.append(out)
        out, mcols = _nan(c.nval), torch.zeros_like(c.cols)
        g.lod_mass_matrix(np.arange(NP), c.slab[k][0].data_ptr(), c.stride, out.data_ptr(), mcols.data_ptr())
        c.mass.append(out)
    c.load = torch.zeros(c.field, dtype=torch.float64, device=dev)
    g.fem_rhs(None, c.load.data_ptr())
    c.rhs = []
    for k in range(c.K):
        out = _nan(c.nrow)
        g.lod_rhs(np.arange(NP), c.slab[k][0].data_ptr(), c.stride, c.load.data_ptr(), out.data_ptr())
        c.rhs.append(out)
    torch.cuda.synchronize()
    c.dA = [_dense(c, v) for v in c.sym]
    c.dM = [_dense(c, v) for v in c.mass]
    lam = [sl.eigh(c.dA[k], c.dM[k], eigvals_only=True) for k in range(c.K)]
    c.w1 = max(math.sqrt(l[0]) for l in lam)
    c.wmax = max(math.sqrt(l[-1]) for l in lam)
    c.mscale = float(torch.stack(c.mass).abs().max())
    _cache[name] = c
    return c


def _dt(c, beta):
    return 0.7 / c.w1 if beta == 0.25 else 1.8 / c.wmax


def _stack(c, mats, K, pad=0):
    """K matrices interleaved [nval][K + pad], NaN in the padding: the three members, then (1 + k/64) member[k mod 3]."""
    torch, dev = _torch()
    f = [1.0 if k < c.K else 1.0 + k / 64.0 for k in range(K)]
    V = _nan(c.nval, K + pad)
    V[:, :K] = torch.stack([mats[k % c.K] * f[k] for k in range(K)], dim=1)
    return V


def _dense(c, values):
    return _rows_to_dense(c.g, values.contiguous().cpu().numpy(), c.hcols, c.s)


def _col(T, k):
    """Column k as a single-problem vector [nrow][1]."""
    return T[:, k:k + 1].contiguous()


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def _combined(c, A, M, K, alpha, beta):
    """S = alpha M + beta A by the ensemble combination, its ensemble factor, and per member (A_k, M_k, single factor of
    S_k), S_k by the single combination: the same words."""
    torch, dev = _torch()
    g, cols = c.g, c.cols.data_ptr()
    S = _nan(c.nval, K)
    g.lod_matrix_combine_ensemble(alpha, M.data_ptr(), beta, A.data_ptr(), K, S.data_ptr(), ld_a=M.shape[1], ld_b=A.shape[1])
    torch.cuda.synchronize()
    f = g.lod_factor_ensemble(S.data_ptr(), cols, K)
    singles = []
    for k in range(K):
        Ak, Mk, Sk = A[:, k].contiguous(), M[:, k].contiguous(), _nan(c.nval)
        g.lod_matrix_combine(alpha, Mk.data_ptr(), beta, Ak.data_ptr(), Sk.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Sk), _bits(S[:, k]))
        singles.append((Ak, Mk, g.lod_factor(Sk.data_ptr(), cols)))
    return f, singles


def _close(f, singles):
    for _, _, fk in singles:
        fk.close()
    f.close()


# ---- 1. the bilinear form

@pytest.mark.parametrize("name,K", CASES)
def test_inner_ensemble_equals_single_calls(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    g, cols = c.g, c.cols.data_ptr()
    rng = np.random.default_rng(301)
    X, Y = _padded(rng.uniform(-1.0, 1.0, (c.nrow, K)), 1), _padded(rng.uniform(-1.0, 1.0, (c.nrow, K)), 3)
    for label, mats in (("sym(A)", c.sym), ("M", c.mass)):
        V = _stack(c, mats, K, pad=2)
        torch.cuda.synchronize()
        wide = g.lod_inner_ensemble(V.data_ptr(), cols, X.data_ptr(), Y.data_ptr(), K, ld_m=K + 2, ld_x=K + 1, ld_y=K + 3)
        quad = g.lod_inner_ensemble(V.data_ptr(), cols, Y.data_ptr(), Y.data_ptr(), K, ld_m=K + 2, ld_x=K + 3, ld_y=K + 3)
        assert np.isfinite(wide).all() and np.isfinite(quad).all() and (quad > 0.0).all()
        for k in range(K):
            Vk, xk, yk = V[:, k].contiguous(), _col(X, k), _col(Y, k)
            one = g.lod_inner(Vk.data_ptr(), cols, xk.data_ptr(), yk.data_ptr())
            assert wide[k:k + 1].tobytes() == one.tobytes(), (name, label, K, k)
            one = g.lod_inner(Vk.data_ptr(), cols, yk.data_ptr(), yk.data_ptr())
            assert quad[k:k + 1].tobytes() == one.tobytes(), (name, label, K, k)
        if K == c.K:                                                 # the value, against the dense form
            hx, hy = X.cpu().numpy(), Y.cpu().numpy()
            for k in range(K):
                exact = float(hx[:, k] @ (_dense(c, V[:, k]) @ hy[:, k]))
                scale = float(np.abs(hx[:, k]) @ (np.abs(_dense(c, V[:, k])) @ np.abs(hy[:, k])))
                assert abs(wide[k] - exact) <= 1e-12 * scale
        # a repeated call
        assert g.lod_inner_ensemble(V.data_ptr(), cols, X.data_ptr(), Y.data_ptr(), K, ld_m=K + 2, ld_x=K + 1,
                                    ld_y=K + 3).tobytes() == wide.tobytes()
        # a member sub-range: base + first member
        sub = g.lod_inner_ensemble(V.data_ptr() + 8, cols, X.data_ptr() + 8, Y.data_ptr() + 8, K - 1, ld_m=K + 2, ld_x=K + 1,
                                   ld_y=K + 3)
        assert sub.tobytes() == wide[1:].tobytes()
        # permuted members give permuted results
        perm = rng.permutation(K)
        tp = torch.from_numpy(perm).to(dev)
        Vp, Xp, Yp = V[:, tp].contiguous(), X[:, tp].contiguous(), Y[:, tp].contiguous()
        got = g.lod_inner_ensemble(Vp.data_ptr(), cols, Xp.data_ptr(), Yp.data_ptr(), K)
        assert got.tobytes() == wide[perm].tobytes()
        assert torch.isnan(V[:, K:]).all() and torch.isnan(X[:, K:]).all() and torch.isnan(Y[:, K:]).all()


# ---- 2. the initial acceleration

@pytest.mark.parametrize("name,K", CASES)
def test_accel_ensemble_direct_equals_single_calls(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    g, cols = c.g, c.cols.data_ptr()
    rng = np.random.default_rng(303)
    u0, v0 = rng.uniform(-1.0, 1.0, (c.nrow, K)), rng.uniform(-1.0, 1.0, (c.nrow, K)) * c.w1
    b0 = rng.uniform(-1.0, 1.0, (c.nrow, K)) * c.mscale
    A, M = _stack(c, c.sym, K, pad=1), _stack(c, c.mass, K, pad=2)   # ld_a_m != ld_m_m
    f, singles = _combined(c, A, M, K, 1.0, 0.0)                     # the factors of M (M + 0 A has the words of M)
    assert np.array_equal(_bits(M[:, 0]), _bits(c.mass[0]))
    U, V, B = _padded(u0, 1), _padded(v0, 2), _padded(b0, 1)
    worst = 0.0
    for dm, ds in ((0.0, 0.0), DAMPED):
        for loaded in (False, True):
            Acc = _nan(c.nrow, K + 3)
            g.lod_newmark_accel_ensemble_direct(f, A.data_ptr(), M.data_ptr(), cols, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr(),
                                                ld_a_m=K + 1, ld_m_m=K + 2, ld_u=K + 1, ld_v=K + 2, ld_a=K + 3,
                                                d_load=B.data_ptr() if loaded else None, ld_load=K + 1, damp_mass=dm, damp_stiff=ds)
            assert torch.isfinite(Acc[:, :K]).all() and torch.isnan(Acc[:, K:]).all()
            for k in range(K):
                Ak, Mk, fk = singles[k]
                uk, vk, bk, ak = _col(U, k), _col(V, k), _col(B, k), _nan(c.nrow, 1)
                g.lod_newmark_accel_direct(fk, Ak.data_ptr(), Mk.data_ptr(), cols, uk.data_ptr(), vk.data_ptr(), ak.data_ptr(),
                                           d_load=bk.data_ptr() if loaded else None, damp_mass=dm, damp_stiff=ds)
                assert np.array_equal(_bits(Acc[:, k]), _bits(ak[:, 0])), (name, K, dm, loaded, k)
            if K == c.K:                                             # against the dense solve per member
                ha = Acc[:, :K].cpu().numpy()
                for k in range(K):
                    rhs = (b0[:, k] if loaded else 0.0) - c.dA[k] @ (u0[:, k] + ds * v0[:, k]) - dm * (c.dM[k] @ v0[:, k])
                    err = _rel(ha[:, k], np.linalg.solve(c.dM[k], rhs))
                    worst = max(worst, err)
                    assert err <= 1e-8, (name, dm, loaded, k, err)
    assert torch.isnan(U[:, K:]).all() and torch.isnan(V[:, K:]).all() and torch.isnan(B[:, K:]).all()
    assert torch.isnan(A[:, K:]).all() and torch.isnan(M[:, K:]).all()
    if K == c.K:
        print("%s: acceleration on an ensemble factor, worst deviation from the dense solve %.3e of max |a|" % (name, worst))
    _close(f, singles)


# ---- 3. the stepper

def _model_steps(A, M, dt, beta, gamma, n_steps, u, v, a, loads, damp):
    """The dense recursion of one member; loads(j) = b^j."""
    Cd = damp[0] * M + damp[1] * A
    S = M + gamma * dt * Cd + beta * dt * dt * A
    for j in range(n_steps):
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        a = np.linalg.solve(S, loads(j + 1) - A @ ut - Cd @ vt)
        u = ut + beta * dt * dt * a
        v = vt + gamma * dt * a
    return u, v, a


def _start(c, K, seed):
    """A state (u, v) per member and the consistent acceleration by the ensemble call (checked above): host arrays."""
    torch, dev = _torch()
    g, cols = c.g, c.cols.data_ptr()
    rng = np.random.default_rng(seed)
    u0, v0 = rng.uniform(-1.0, 1.0, (c.nrow, K)), rng.uniform(-1.0, 1.0, (c.nrow, K)) * c.w1
    A, M = _stack(c, c.sym, K), _stack(c, c.mass, K)
    fM = g.lod_factor_ensemble(M.data_ptr(), cols, K)
    U, V, Acc = _dev(u0), _dev(v0), _nan(c.nrow, K)
    g.lod_newmark_accel_ensemble_direct(fM, A.data_ptr(), M.data_ptr(), cols, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr())
    fM.close()
    return u0, v0, Acc.cpu().numpy()


@pytest.mark.parametrize("name,K", CASES)
def test_newmark_steps_ensemble_direct_equals_single_steppers(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    g, cols, steps, gamma = c.g, c.cols.data_ptr(), 3, 0.5
    u0, v0, a0 = _start(c, K, 305)
    L = np.random.default_rng(307).uniform(-1.0, 1.0, (steps + 1, c.nrow, K)) * c.mscale
    Lt = _nan(steps + 1, c.nrow, K + 1)                              # padded ld_load
    Lt[:, :, :K] = _dev(L)
    A, M = _stack(c, c.sym, K, pad=1), _stack(c, c.mass, K, pad=2)   # ld_a_m != ld_m_m
    small = K == c.K
    worst = 0.0
    for beta, damp in ((0.25, (0.0, 0.0)), (0.25, DAMPED), (0.0, (0.0, 0.0))) if small else ((0.25, (0.0, 0.0)), (0.25, DAMPED)):
        dt = _dt(c, beta)
        f, singles = _combined(c, A, M, K, 1.0 + gamma * dt * damp[0], beta * dt * dt + gamma * dt * damp[1])
        for loading in ("none", "constant", "distinct") if small else ("constant",):
            load, stride, loads = {"none": (None, 0, lambda j: np.zeros((c.nrow, K))),
                                   "constant": (Lt[1], 0, lambda j: L[1]),
                                   "distinct": (Lt, c.nrow * (K + 1), lambda j: L[j])}[loading]

            def run(n_steps, U, V, Acc, energies, first=0):
                return g.lod_newmark_steps_ensemble_direct(
                    f, A.data_ptr(), M.data_ptr(), cols, dt, n_steps, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr(), beta=beta,
                    gamma=gamma, ld_a_m=K + 1, ld_m_m=K + 2, ld_u=U.shape[1], ld_v=V.shape[1], ld_a=Acc.shape[1],
                    d_load=None if load is None else load.data_ptr() + 8 * first * stride, ld_load=K + 1, load_step_stride=stride,
                    damp_mass=damp[0], damp_stiff=damp[1], energies=energies)

            U, V, Acc = _padded(u0, 1), _padded(v0, 2), _padded(a0, 3)
            kin, pot = run(steps, U, V, Acc, True)
            assert kin.shape == pot.shape == (steps + 1, K) and np.isfinite(kin).all() and np.isfinite(pot).all()
            for T in (U, V, Acc):
                assert torch.isfinite(T[:, :K]).all() and torch.isnan(T[:, K:]).all()
            # the energies change no state, and a repeated call gives the same words
            U2, V2, A2 = _padded(u0, 2), _padded(v0, 1), _padded(a0, 1)
            assert run(steps, U2, V2, A2, False) == (None, None)
            for T, T2 in ((U, U2), (V, V2), (Acc, A2)):
                assert np.array_equal(_bits(T[:, :K]), _bits(T2[:, :K])) and torch.isnan(T2[:, K:]).all()
            U2, V2, A2 = _padded(u0, 1), _padded(v0, 2), _padded(a0, 3)
            kin2, pot2 = run(steps, U2, V2, A2, True)
            assert kin2.tobytes() == kin.tobytes() and pot2.tobytes() == pot.tobytes()
            assert np.array_equal(_bits(U2), _bits(U)) and np.array_equal(_bits(V2), _bits(V)) and np.array_equal(_bits(A2), _bits(Acc))
            # the single steppers
            for k in range(K):
                Ak, Mk, fk = singles[k]
                u, v, a = _dev(u0[:, k:k + 1]), _dev(v0[:, k:k + 1]), _dev(a0[:, k:k + 1])
                Lk = None if load is None else (Lt[:, :, k].contiguous() if loading == "distinct" else Lt[1, :, k].contiguous())
                k1, p1 = g.lod_newmark_steps_direct(fk, Ak.data_ptr(), Mk.data_ptr(), cols, dt, steps, u.data_ptr(), v.data_ptr(),
                                                    a.data_ptr(), beta=beta, gamma=gamma,
                                                    d_load=None if Lk is None else Lk.data_ptr(),
                                                    load_step_stride=c.nrow if stride else 0, damp_mass=damp[0], damp_stiff=damp[1])
                where = (name, K, beta, damp, loading, k)
                assert np.array_equal(_bits(U[:, k]), _bits(u[:, 0])), where
                assert np.array_equal(_bits(V[:, k]), _bits(v[:, 0])), where
                assert np.array_equal(_bits(Acc[:, k]), _bits(a[:, 0])), where
                assert kin[:, k].tobytes() == k1[:, 0].tobytes() and pot[:, k].tobytes() == p1[:, 0].tobytes(), where
            if small:                                                # against the dense recursion per member
                hu, hv, ha = (T[:, :K].cpu().numpy() for T in (U, V, Acc))
                for k in range(K):
                    ru, rv, ra = _model_steps(c.dA[k], c.dM[k], dt, beta, gamma, steps, u0[:, k], v0[:, k], a0[:, k],
                                              lambda j: loads(j)[:, k], damp)
                    err = max(_rel(hu[:, k], ru), _rel(hv[:, k], rv), _rel(ha[:, k], ra))
                    worst = max(worst, err)
                    assert err <= 1e-8, (name, beta, damp, loading, k, err)
            if loading != "none":
                # n_steps = 2 equals 2 x n_steps = 1 carrying u, v, a over, as words
                Ua, Va, Aa = _dev(u0), _dev(v0), _dev(a0)
                ka, pa = run(2, Ua, Va, Aa, True)
                Ub, Vb, Ab = _dev(u0), _dev(v0), _dev(a0)
                kb0, pb0 = run(1, Ub, Vb, Ab, True)
                kb1, pb1 = run(1, Ub, Vb, Ab, True, first=1)
                for Ta, Tb in ((Ua, Ub), (Va, Vb), (Aa, Ab)):
                    assert np.array_equal(_bits(Ta), _bits(Tb)), (name, K, beta, damp, loading)
                assert ka.tobytes() == np.vstack([kb0, kb1[1:]]).tobytes() and pa.tobytes() == np.vstack([pb0, pb1[1:]]).tobytes()
                assert kb1[0].tobytes() == kb0[1].tobytes()
        _close(f, singles)
    assert torch.isnan(A[:, K:]).all() and torch.isnan(M[:, K:]).all() and torch.isnan(Lt[:, :, K:]).all()
    if small:
        print("%s: Newmark steps on an ensemble factor, worst deviation from the dense recursion %.3e of max |reference|"
              % (name, worst))


def test_newmark_ensemble_skips_the_mass_product_without_mass_damping(so):
    """damp_mass = 0: a d_mass full of NaN leaves the state finite and with the words of the run on M (the mass product of
    the per-column k_nm_rhs is skipped, as in the single call; the damped cases above run it).  The energies are off:
    the kinetic energy does read M."""
    torch, dev = _torch()
    c = _case(so, "rowmajor")
    g, cols, K, steps = c.g, c.cols.data_ptr(), c.K, 3
    u0, v0, a0 = _start(c, K, 309)
    A, M, bad = _stack(c, c.sym, K), _stack(c, c.mass, K), _nan(c.nval, K)
    dt, ds = _dt(c, 0.25), DAMPED[1]
    f, singles = _combined(c, A, M, K, 1.0, 0.25 * dt * dt + 0.5 * dt * ds)
    fM = g.lod_factor_ensemble(M.data_ptr(), cols, K)
    out = []
    for mass in (M, bad):
        U, V, Acc, A0 = _dev(u0), _dev(v0), _dev(a0), _nan(c.nrow, K)
        g.lod_newmark_accel_ensemble_direct(fM, A.data_ptr(), mass.data_ptr(), cols, K, U.data_ptr(), V.data_ptr(), A0.data_ptr(),
                                            damp_stiff=ds)
        assert g.lod_newmark_steps_ensemble_direct(f, A.data_ptr(), mass.data_ptr(), cols, dt, steps, K, U.data_ptr(), V.data_ptr(),
                                                   Acc.data_ptr(), damp_stiff=ds, energies=False) == (None, None)
        for T in (U, V, Acc, A0):
            assert torch.isfinite(T).all()
        out.append([_bits(T) for T in (U, V, Acc, A0)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    fM.close()
    _close(f, singles)


# ---- 4. conservation and decay

def test_newmark_ensemble_trapezoidal_conserves_energy_and_damping_dissipates(so):
    torch, dev = _torch()
    c = _case(so, "base")
    g, cols, K, steps = c.g, c.cols.data_ptr(), c.K, 10
    dt = _dt(c, 0.25)
    u0 = np.random.default_rng(311).uniform(-1.0, 1.0, (c.nrow, K))
    A, M = _stack(c, c.sym, K), _stack(c, c.mass, K)
    fM = g.lod_factor_ensemble(M.data_ptr(), cols, K)
    for dm, ds in ((0.0, 0.0), DAMPED):
        S = _nan(c.nval, K)
        g.lod_matrix_combine_ensemble(1.0 + 0.5 * dt * dm, M.data_ptr(), 0.25 * dt * dt + 0.5 * dt * ds, A.data_ptr(), K, S.data_ptr())
        torch.cuda.synchronize()
        f = g.lod_factor_ensemble(S.data_ptr(), cols, K)
        U, V, Acc = _dev(u0), torch.zeros(c.nrow, K, dtype=torch.float64, device=dev), _nan(c.nrow, K)
        g.lod_newmark_accel_ensemble_direct(fM, A.data_ptr(), M.data_ptr(), cols, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr(),
                                            damp_mass=dm, damp_stiff=ds)
        kin, pot = g.lod_newmark_steps_ensemble_direct(f, A.data_ptr(), M.data_ptr(), cols, dt, steps, K, U.data_ptr(), V.data_ptr(),
                                                       Acc.data_ptr(), damp_mass=dm, damp_stiff=ds)
        E = kin + pot
        for k in range(K):
            drift = np.abs(E[:, k] - E[0, k]).max() / E[0, k]
            print("member %d, damping (%g, %g): kinetic + potential over %d trapezoidal steps from %.9e to %.9e, largest relative "
                  "change %.3e" % (k, dm, ds, steps, E[0, k], E[-1, k], drift))
            assert E[0, k] > 0.0 and kin[0, k] == 0.0
            assert E[0, k] == pytest.approx(0.5 * float(u0[:, k] @ c.dA[k] @ u0[:, k]), rel=1e-12)
            if dm == 0.0:
                assert drift <= 1e-8, (k, drift)
            else:
                assert (E[1:, k] <= E[:-1, k] + 1e-12 * E[:-1, k]).all() and E[-1, k] < E[0, k], (k, E[:, k])
        f.close()
    fM.close()


# ---- 5. refusals that need a factor

def test_newmark_ensemble_direct_refuses_another_member_count(so):
    import slod_amd
    torch, dev = _torch()
    c = _case(so, "rowmajor")
    g, K, cols = c.g, c.K, c.cols.data_ptr()
    A, M = _stack(c, c.sym, K), _stack(c, c.mass, K)
    f3 = g.lod_factor_ensemble(M.data_ptr(), cols, K)
    f1 = g.lod_factor(c.mass[0].data_ptr(), cols)
    u, v, a = (torch.zeros(c.nrow, K, dtype=torch.float64, device=dev) for _ in range(3))
    p = (u.data_ptr(), v.data_ptr(), a.data_ptr())
    lds = dict(ld_a_m=K, ld_m_m=K, ld_u=K, ld_v=K, ld_a=K)
    calls = (lambda: g.lod_newmark_steps_ensemble_direct(f3, A.data_ptr(), M.data_ptr(), cols, 0.01, 1, K - 1, *p, **lds),
             lambda: g.lod_newmark_steps_ensemble_direct(f1, A.data_ptr(), M.data_ptr(), cols, 0.01, 1, K, *p),
             lambda: g.lod_newmark_accel_ensemble_direct(f3, A.data_ptr(), M.data_ptr(), cols, K - 1, *p, **lds),
             lambda: g.lod_newmark_accel_ensemble_direct(f1, A.data_ptr(), M.data_ptr(), cols, K, *p),
             # the single calls on the factor of three members stay refused
             lambda: g.lod_newmark_steps_direct(f3, c.sym[0].data_ptr(), c.mass[0].data_ptr(), cols, 0.01, 1, *p, ld_u=K, ld_v=K, ld_a=K),
             lambda: g.lod_newmark_accel_direct(f3, c.sym[0].data_ptr(), c.mass[0].data_ptr(), cols, *p, ld_u=K, ld_v=K, ld_a=K))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and "factor of another member count" in str(e.value)
    other = _case(so, "base")
    with pytest.raises(slod_amd.SlodError) as e:
        other.g.lod_newmark_steps_ensemble_direct(f3, A.data_ptr(), M.data_ptr(), cols, 0.01, 1, K, *p)
    assert e.value.code == -1 and "factor of another handle" in str(e.value)
    torch.cuda.synchronize()
    assert (u == 0.0).all() and (v == 0.0).all() and (a == 0.0).all()
    f1.close()
    f3.close()


# ---- 6. end to end

def _moments_numpy(x):
    K = x.shape[0]
    total = x[0].copy()
    for k in range(1, K):
        total = total + x[k]
    mean = total / np.float64(K)
    acc = np.zeros_like(mean)
    for k in range(K):
        d = x[k] - mean
        acc = acc + d * d
    return mean, acc / np.float64(K - 1)


def test_wave_pipeline_equals_three_single_pipelines(so):
    torch, dev = _torch()
    c = _case(so, "base")
    g, K, steps, beta, gamma = c.g, c.K, 4, 0.25, 0.5
    dt = _dt(c, beta)
    V, M, A, S = _nan(c.nval, K), _nan(c.nval, K), _nan(c.nval, K), _nan(c.nval, K)
    cols, mcols = torch.zeros_like(c.cols), torch.zeros_like(c.cols)
    R, fine = _nan(c.nrow, K), _nan(K, c.field)
    Ut, Vt = (torch.zeros(c.nrow, K, dtype=torch.float64, device=dev) for _ in range(2))
    At = _nan(c.nrow, K)
    mean, var = _nan(c.field), _nan(c.field)
    torch.cuda.synchronize()
    g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix_ensemble(c.b.data_ptr(), c.stride, K, M.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, A.data_ptr())
    g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), beta * dt * dt, A.data_ptr(), K, S.data_ptr())
    g.lod_rhs_ensemble(c.b.data_ptr(), c.stride, K, c.load.data_ptr(), R.data_ptr())
    fM = g.lod_factor_ensemble(M.data_ptr(), cols.data_ptr(), K)
    fS = g.lod_factor_ensemble(S.data_ptr(), cols.data_ptr(), K)
    g.lod_newmark_accel_ensemble_direct(fM, A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, Ut.data_ptr(), Vt.data_ptr(), At.data_ptr(),
                                        d_load=R.data_ptr())
    kin, pot = g.lod_newmark_steps_ensemble_direct(fS, A.data_ptr(), M.data_ptr(), cols.data_ptr(), dt, steps, K, Ut.data_ptr(),
                                                   Vt.data_ptr(), At.data_ptr(), beta=beta, gamma=gamma, d_load=R.data_ptr())
    g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, K, Ut.data_ptr(), fine.data_ptr())
    g.ensemble_moments(fine.data_ptr(), K, c.field, mean.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(cols, c.cols) and torch.equal(mcols, c.cols)
    single = []
    for k in range(K):
        Sk = _nan(c.nval)
        g.lod_matrix_combine(1.0, c.mass[k].data_ptr(), beta * dt * dt, c.sym[k].data_ptr(), Sk.data_ptr())
        torch.cuda.synchronize()
        fMk, fSk = g.lod_factor(c.mass[k].data_ptr(), c.cols.data_ptr()), g.lod_factor(Sk.data_ptr(), c.cols.data_ptr())
        u, v = (torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev) for _ in range(2))
        a = _nan(c.nrow, 1)
        g.lod_newmark_accel_direct(fMk, c.sym[k].data_ptr(), c.mass[k].data_ptr(), c.cols.data_ptr(), u.data_ptr(), v.data_ptr(),
                                   a.data_ptr(), d_load=c.rhs[k].data_ptr())
        k1, p1 = g.lod_newmark_steps_direct(fSk, c.sym[k].data_ptr(), c.mass[k].data_ptr(), c.cols.data_ptr(), dt, steps, u.data_ptr(),
                                            v.data_ptr(), a.data_ptr(), beta=beta, gamma=gamma, d_load=c.rhs[k].data_ptr())
        out = _nan(c.field)
        g.lod_reconstruct(c.slab[k][0].data_ptr(), c.stride, u.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        for T, t in ((Ut, u), (Vt, v), (At, a)):
            assert np.array_equal(_bits(T[:, k]), _bits(t[:, 0])), k
        assert kin[:, k].tobytes() == k1[:, 0].tobytes() and pot[:, k].tobytes() == p1[:, 0].tobytes(), k
        single.append(out.cpu().numpy())
        fMk.close()
        fSk.close()
    single = np.stack(single)
    assert np.array_equal(_bits(fine), single.view(np.uint64))
    m, v = _moments_numpy(single)
    assert np.array_equal(_bits(mean), m.view(np.uint64)) and np.array_equal(_bits(var), v.view(np.uint64))
    assert np.isfinite(single).all() and v.max() > 0.0 and np.abs(m).max() > 0.0 and (kin[1:] > 0.0).all()
    fM.close()
    fS.close()


# ---- 7. the driver

def _driver(*args):
    """A fresh child process per run, under its own timeout; the driver's default configuration (3 4 1 1)."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_driver_ensemble_wave_direct():
    """main_Diffusion --ensemble 3 --wave 4 0.005 --direct: the energy lines of member k are those of a single
    --member k --wave 4 0.005 --direct run, to the digits printed; from rest under a constant load the trapezoidal rule
    keeps kinetic + potential - work = 0."""
    K, steps = 3, 4
    out = _driver("--ensemble", str(K), "--wave", str(steps), "0.005", "--direct")
    lines = re.findall(r"^member (\d+) wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", out, re.M)
    assert [(int(a), int(b)) for a, b, _, _, _ in lines] == [(k, j) for k in range(K) for j in range(1, steps + 1)], out
    ens = {(int(a), int(b)): (kin, pot, work) for a, b, kin, pot, work in lines}
    factor = re.findall(r"^factor: n = (\d+), half bandwidth = (\d+), bytes = (\d+), pivots in \[(\S+), (\S+)\]$", out, re.M)
    assert len(factor) == 2 and factor[0][:2] == factor[1][:2]                          # member 0 alone, then the ensemble
    assert int(factor[1][2]) > (K - 1) * int(factor[0][2]) and float(factor[1][3]) > 0.0
    m = re.search(r"^SLOD wave ensemble of 3 at T = 0.02: L2 norm of the mean = (\S+), of the standard deviation = (\S+)$", out, re.M)
    assert m and float(m.group(1)) > 0.0 and float(m.group(2)) > 0.0, out
    for k in range(K):
        one = _driver("--member", str(k), "--wave", str(steps), "0.005", "--direct")
        rows = re.findall(r"^wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", one, re.M)
        assert [int(r[0]) for r in rows] == list(range(1, steps + 1)), one
        for j, kin, pot, work in rows:
            assert ens[(k, int(j))] == (kin, pot, work), (k, j, ens[(k, int(j))], (kin, pot, work))
        kin, pot, work = (np.array([float(ens[(k, j)][i]) for j in range(1, steps + 1)]) for i in range(3))
        gap = np.abs(kin + pot - work).max() / pot.max()
        print("member %d: largest |kinetic + potential - work| / max potential %.3e" % (k, gap))
        assert (kin > 0).all() and (pot > 0).all() and gap <= 1e-8, (k, kin, pot, work)
    assert len({ens[(k, steps)] for k in range(K)}) == K            # the members differ
    # member 0 of the ensemble is the run's own coefficient: its lines repeat those of the single loop printed before
    own = re.findall(r"^wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", out, re.M)
    assert [ens[(0, int(j))] for j, _, _, _ in own] == [r[1:] for r in own] and len(own) == steps
