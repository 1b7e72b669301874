"""Ensemble time stepping on banded Cholesky factors on the GPU: the mass matrix, the symmetrised stiffness and the
combinations of every member, the factor object that holds a factor per member, its solves and the theta scheme with one
column per member.  Every comparison is one of 64-bit words against the single-problem call on the de-interleaved member
unless it says otherwise.

Configurations (those of test_gpu_lod_ensemble.py, built the same way: one handle with n_problems = 3, members const /
D100 / D1e4 of make_fields, one plan over all 3 * num_patches gids; n rows, half bandwidth b):
  base      nref 3, n_sub 2, l 1, s 1   n = 64,  b = 27   nb = 4 > bb + 1 = 3: the band is truncated
  s2        nref 3, n_sub 2, l 1, s 2   n = 128, b = 55   elasticity
  rowmajor  5 cells, n_sub 3, l 1       n = 25,  b = 18   padding in n and in b, row-major ids
K = 65 takes the scaled copies (1 + k/64) member[k mod 3] (a positive scale keeps them positive definite) and crosses a
wave of members; K = 17 with n_rhs = 17 crosses the 16-column tile of the solve.

Bars that are not equality of words:
  backward error  eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), residual in np.longdouble, at most
                  (3 (b + 1) + 1) (b + 1) 2^-53, the bar of test_gpu_lod_factor.py
  forward error   1e-8 relative per column against numpy.linalg.solve
  stepper         1e-8 relative against the dense numpy recursion per member
"""
import ctypes as C
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
SHAPE = {"base": (64, 27), "s2": (128, 55), "rowmajor": (25, 18)}    # rows, half bandwidth
NAMES = sorted(CONFIGS)
U = 2.0 ** -53
_cache = {}


class _Ens:
    pass


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _single_mass(c, k, rho=None):
    torch, dev = _torch()
    values = _nan(c.nval)
    cols = torch.zeros(c.NP * c.cap, dtype=torch.int32, device=dev)
    c.g.lod_mass_matrix(np.arange(c.NP), c.slab[k][0].data_ptr(), c.stride, values.data_ptr(), cols.data_ptr(),
                        d_rho=None if rho is None else rho.data_ptr())
    torch.cuda.synchronize()
    return values, cols


def _single_sym(c, values):
    torch, dev = _torch()
    values = values.contiguous()
    out = _nan(c.nval)
    c.g.lod_matrix_symmetrize(values.data_ptr(), c.cols.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def _single_combine(c, alpha, a, beta, b):
    torch, dev = _torch()
    a, b = a.contiguous(), b.contiguous()
    out = _nan(c.nval)
    c.g.lod_matrix_combine(alpha, a.data_ptr(), beta, b.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def _case(so, name):
    """Handle, ensemble slab, and per member the single-problem A, sym(A), M, M + 0.01 sym(A) and load vector (f = 1);
    built once and left unchanged."""
    if name in _cache:
        return _cache[name]
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
    w = 2 * kw["oversampling"] + 1
    c.hbw = c.s * (w * g.N + w) + c.s - 1
    assert (c.nrow, c.hbw) == SHAPE[name]
    c.slab = [(c.b[k * c.mstride:(k + 1) * c.mstride], c.q[k * c.mstride:(k + 1) * c.mstride]) for k in range(c.K)]
    c.values, c.cols = [], None
    for bk, qk in c.slab:
        v, cols = _lod_matrix(g, bk, qk, c.stride, c.s)
        c.values.append(v)
        assert c.cols is None or torch.equal(c.cols, cols)
        c.cols = cols
    c.hcols = c.cols.cpu().numpy().view(np.uint32)
    c.sym = [_single_sym(c, v) for v in c.values]
    c.mass = [_single_mass(c, k)[0] for k in range(c.K)]
    c.mix = [_single_combine(c, 1.0, c.mass[k], 0.01, c.sym[k]) for k in range(c.K)]
    c.mats = {"sym(A)": c.sym, "M": c.mass, "M + 0.01 A": c.mix}
    c.load = torch.zeros(c.field, dtype=torch.float64, device=dev)
    g.fem_rhs(None, c.load.data_ptr())
    c.rhs = []
    for k in range(c.K):
        out = _nan(c.nrow)
        g.lod_rhs(np.arange(NP), c.slab[k][0].data_ptr(), c.stride, c.load.data_ptr(), out.data_ptr())
        c.rhs.append(out)
    torch.cuda.synchronize()
    _cache[name] = c
    return c


def _scale(c, K):
    return [1.0 if k < c.K else 1.0 + k / 64.0 for k in range(K)]


def _stack(c, mats, K, pad=0):
    """K matrices interleaved [nval][K + pad], NaN in the padding: the three members, then (1 + k/64) member[k mod 3]."""
    torch, dev = _torch()
    f = _scale(c, K)
    V = _nan(c.nval, K + pad)
    V[:, :K] = torch.stack([mats[k % c.K] * f[k] for k in range(K)], dim=1)
    return V


def _dense(c, values):
    return _rows_to_dense(c.g, values.contiguous().cpu().numpy(), c.hcols, c.s)


def _eta(A, x, b):
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)
    an = np.abs(A).sum(axis=1).max()
    return np.array(np.abs(r).max(axis=0) / (an * np.abs(x).max(axis=0) + np.abs(b).max(axis=0)), dtype=np.float64)


def _bound(b):
    return (3 * (b + 1) + 1) * (b + 1) * U


def _same_words(a, b):
    return np.array([a]).tobytes() == np.array([b]).tobytes()


# ---- matrices

@pytest.mark.parametrize("rho", ["none", "shared", "per_member"])
@pytest.mark.parametrize("name", NAMES)
def test_mass_ensemble_equals_single_calls(so, name, rho):
    torch, dev = _torch()
    c = _case(so, name)
    K, ne2 = c.K, c.g.NE ** 2
    gen = torch.Generator(device="cpu").manual_seed(17)
    ld_rho = {"none": 0, "shared": 0, "per_member": ne2 + 3}[rho]                # a padded ld_rho
    R = None
    if rho == "shared":
        R = (torch.rand(1, ne2, generator=gen, dtype=torch.float64) + 0.5).to(dev)
    elif rho == "per_member":
        R = _nan(K, ld_rho)
        R[:, :ne2] = (torch.rand(K, ne2, generator=gen, dtype=torch.float64) + 0.5).to(dev)
    ld = K + 2
    V = _nan(c.nval, ld)
    cols = torch.full((c.NP * c.cap,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c.g.lod_mass_matrix_ensemble(c.b.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr(), d_rho=None if R is None else R.data_ptr(),
                                 ld_rho=ld_rho, ld_m=ld)
    torch.cuda.synchronize()
    single_cols = None
    for k in range(K):
        rk = None if R is None else R[k if rho == "per_member" else 0, :ne2].contiguous()
        ref, single_cols = (c.mass[k], c.cols) if R is None else _single_mass(c, k, rk)
        assert np.array_equal(_bits(V[:, k]), _bits(ref)), (name, rho, k)
        assert torch.equal(cols, single_cols)
    assert torch.isnan(V[:, K:]).all()                                            # a padded ld_m keeps its NaN
    assert torch.equal(cols, c.cols)
    if rho != "none":
        assert not np.array_equal(_bits(V[:, 0]), _bits(c.mass[0]))               # the density is read
    assert not torch.equal(V[:, 0], V[:, 1]) and not torch.equal(V[:, 1], V[:, 2])
    # a member sub-range: base + first member
    W = _nan(c.nval, ld)
    c.g.lod_mass_matrix_ensemble(c.b.data_ptr() + 8 * c.mstride, c.stride, K - 1, W.data_ptr() + 8, cols.data_ptr(),
                                 d_rho=None if R is None else R.data_ptr() + 8 * ld_rho, ld_rho=ld_rho, ld_m=ld)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(W[:, 1:K]), _bits(V[:, 1:K]))
    assert torch.isnan(W[:, 0]).all() and torch.isnan(W[:, K:]).all()


@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("name", NAMES)
def test_symmetrize_and_combine_ensemble_equal_single_calls(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    A = _stack(c, c.values, K, pad=1)
    M = _stack(c, c.mass, K)
    S = _nan(c.nval, K + 2)
    torch.cuda.synchronize()
    c.g.lod_matrix_symmetrize_ensemble(A.data_ptr(), c.cols.data_ptr(), K, S.data_ptr(), ld_in=K + 1, ld_out=K + 2)
    torch.cuda.synchronize()
    sym = [c.sym[k] if k < c.K else _single_sym(c, A[:, k]) for k in range(K)]
    for k in range(K):
        assert np.array_equal(_bits(S[:, k]), _bits(sym[k])), (name, K, k)
    assert torch.isnan(S[:, K:]).all() and torch.isnan(A[:, K]).all()
    out = _nan(c.nval, K + 1)
    c.g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), 0.01, S.data_ptr(), K, out.data_ptr(), ld_a=K, ld_b=K + 2, ld_out=K + 1)
    torch.cuda.synchronize()
    for k in range(K):
        ref = c.mix[k] if k < c.K else _single_combine(c, 1.0, M[:, k], 0.01, sym[k])
        assert np.array_equal(_bits(out[:, k]), _bits(ref)), (name, K, k)
    assert torch.isnan(out[:, K]).all()
    # in place on either input, equal leading dimensions
    a = S.clone()
    b = _nan(c.nval, K + 2)
    b[:, :K] = M
    c.g.lod_matrix_combine_ensemble(0.01, a.data_ptr(), 1.0, b.data_ptr(), K, a.data_ptr(), ld_a=K + 2, ld_b=K + 2, ld_out=K + 2)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a[:, :K]), _bits(out[:, :K])) and torch.isnan(a[:, K:]).all()      # the sum commutes
    c.g.lod_matrix_combine_ensemble(0.01, S.data_ptr(), 1.0, b.data_ptr(), K, b.data_ptr(), ld_a=K + 2, ld_b=K + 2, ld_out=K + 2)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(b[:, :K]), _bits(out[:, :K])) and torch.isnan(b[:, K:]).all()


# ---- factor and solve

def _single_factor_solve(c, values, B, n, first=0):
    """slod_lod_factor_create / _solve on one de-interleaved member: (info, U [nrow][n]); columns first .. of B"""
    torch, dev = _torch()
    values = values.contiguous()
    f = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
    out = _nan(c.nrow, n)
    f.solve(B.data_ptr() + 8 * first, out.data_ptr(), n_rhs=n, ld_rhs=B.shape[1], ld_u=n)
    torch.cuda.synchronize()
    info = (f.info.n, f.info.half_bandwidth, f.info.block, f.info.min_pivot, f.info.max_pivot)
    f.close()
    return info, out


@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("name", NAMES)
def test_factor_ensemble_equals_single_factors(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    B = _dev(np.random.default_rng(201).uniform(-1.0, 1.0, (c.nrow, K)))
    for label, mats in c.mats.items():
        V = _stack(c, mats, K, pad=2)
        f = c.g.lod_factor_ensemble(V.data_ptr(), c.cols.data_ptr(), K, ld_m=K + 2)
        assert (f.bad_pivot == -1).all() and len(f.bad_pivot) == K
        X = _nan(c.nrow, K + 1)
        f.solve(B.data_ptr(), X.data_ptr(), ld_rhs=K, ld_u=K + 1)
        torch.cuda.synchronize()
        lo, hi = [], []
        for k in range(K):
            (n, b, blk, pmin, pmax), x = _single_factor_solve(c, V[:, k], B, 1, first=k)
            mi = f.member_info(k)
            assert (mi.n, mi.half_bandwidth, mi.block) == (n, b, blk) == (c.nrow, c.hbw, 16)
            assert _same_words(mi.min_pivot, pmin) and _same_words(mi.max_pivot, pmax), (name, label, K, k)
            assert mi.bytes == f.info.bytes
            assert np.array_equal(_bits(X[:, k]), _bits(x[:, 0])), (name, label, K, k)
            lo.append(pmin), hi.append(pmax)
        assert torch.isnan(X[:, K]).all() and torch.isnan(V[:, K:]).all()
        assert _same_words(f.info.min_pivot, min(lo)) and _same_words(f.info.max_pivot, max(hi)) and f.info.min_pivot > 0.0
        print("%s %s K = %d: bytes %d (%d per member), pivots [%.3e, %.3e]"
              % (name, label, K, f.info.bytes, f.info.bytes // K, f.info.min_pivot, f.info.max_pivot))
        f.close()


@pytest.mark.parametrize("K,n", [(3, 1), (3, 3), (3, 17), (17, 17)])
@pytest.mark.parametrize("name", NAMES)
def test_factor_solve_ensemble_windows(so, name, K, n):
    torch, dev = _torch()
    c = _case(so, name)
    V = _stack(c, c.mix, K)
    f = c.g.lod_factor_ensemble(V.data_ptr(), c.cols.data_ptr(), K)
    hb = np.random.default_rng(203).uniform(-1.0, 1.0, (c.nrow, K * n))
    B = _dev(hb)
    X = _nan(c.nrow, K * n)
    f.solve(B.data_ptr(), X.data_ptr(), n_rhs=n)
    torch.cuda.synchronize()
    ref = _bits(X)
    hx = X.cpu().numpy()
    for k in range(K):                                               # member k solves its window of n columns
        _, x = _single_factor_solve(c, V[:, k], B, n, first=k * n)
        assert np.array_equal(ref[:, k * n:(k + 1) * n], _bits(x)), (name, K, n, k)
        if k < c.K or k == K - 1:
            A = _dense(c, V[:, k])
            w = slice(k * n, (k + 1) * n)
            eta, sol = _eta(A, hx[:, w], hb[:, w]), np.linalg.solve(A, hb[:, w])
            fwd = np.abs(hx[:, w] - sol).max(axis=0) / np.abs(sol).max(axis=0)
            print("%s K = %d n_rhs = %d member %d: backward error %.3e (bound %.3e), forward error %.3e"
                  % (name, K, n, k, eta.max(), _bound(c.hbw), fwd.max()))
            assert (eta <= _bound(c.hbw)).all(), (name, k, eta.max(), _bound(c.hbw))
            assert (fwd <= 1e-8).all(), (name, k, fwd.max())
    # a repeated solve
    Y = _nan(c.nrow, K * n)
    f.solve(B.data_ptr(), Y.data_ptr(), n_rhs=n)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref)
    # padded leading dimensions, NaN padding left untouched
    Bw = _nan(c.nrow, K * n + 5)
    Bw[:, :K * n] = B
    Y = _nan(c.nrow, K * n + 7)
    f.solve(Bw.data_ptr(), Y.data_ptr(), n_rhs=n, ld_rhs=K * n + 5, ld_u=K * n + 7)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y[:, :K * n]), ref) and torch.isnan(Y[:, K * n:]).all() and torch.isnan(Bw[:, K * n:]).all()
    # in place
    Y = B.clone()
    f.solve(Y.data_ptr(), Y.data_ptr(), n_rhs=n)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref)
    # a sub-range of the members: first_member > 0, base pointers at its first column
    first, cnt = 1, K - 2 if K > 3 else K - 1
    Y = _nan(c.nrow, K * n)
    f.solve(B.data_ptr() + 8 * first * n, Y.data_ptr() + 8 * first * n, n_rhs=n, first_member=first, n_members=cnt, ld_rhs=K * n,
            ld_u=K * n)
    torch.cuda.synchronize()
    w = slice(first * n, (first + cnt) * n)
    assert np.array_equal(_bits(Y[:, w]), ref[:, w])
    assert torch.isnan(Y[:, :first * n]).all() and torch.isnan(Y[:, (first + cnt) * n:]).all()
    # permuted members give permuted results
    perm = np.random.default_rng(205).permutation(K)
    colperm = np.concatenate([np.arange(p * n, (p + 1) * n) for p in perm])
    tp = torch.from_numpy(perm).to(dev)
    f2 = c.g.lod_factor_ensemble(V[:, tp].contiguous().data_ptr(), c.cols.data_ptr(), K)
    Y = _nan(c.nrow, K * n)
    f2.solve(B[:, torch.from_numpy(colperm).to(dev)].contiguous().data_ptr(), Y.data_ptr(), n_rhs=n)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref[:, colperm])
    # the refusals that need a factor
    lib = c.g.lib
    bad = ((0, K + 1, K * n, n), (1, K, K * n, n), (-1, 1, K * n, n), (0, 0, K * n, n), (0, K, K * n - 1, n), (0, K, K * n, 0))
    for first_member, members, ld, n_rhs in bad:
        assert lib.slod_lod_factor_solve_ensemble(f.f, first_member, members, B.data_ptr(), ld, n_rhs, X.data_ptr(), K * n, None) == -1
        assert "slod_lod_factor_solve_ensemble" in lib.slod_last_error(c.g.h).decode()
    assert lib.slod_lod_factor_solve_ensemble(f.f, 0, K, None, K * n, n, X.data_ptr(), K * n, None) == -1     # a NULL array
    assert lib.slod_lod_factor_solve_ensemble(f.f, 0, K, B.data_ptr(), K * n, n, None, K * n, None) == -1
    assert "slod_lod_factor_solve_ensemble" in lib.slod_last_error(c.g.h).decode()
    assert lib.slod_lod_factor_solve(f.f, B.data_ptr(), K * n, 1, X.data_ptr(), K * n, None) == -1       # K > 1 members
    assert "slod_lod_factor_solve" in lib.slod_last_error(c.g.h).decode()
    info = type(f.info)()
    assert lib.slod_lod_factor_get_info_member(f.f, K, C.byref(info)) == -1 and lib.slod_lod_factor_get_info_member(f.f, -1, C.byref(info)) == -1
    assert np.array_equal(_bits(X), ref)                                                                  # nothing was written
    f2.close()
    f.close()


def test_single_factor_is_an_ensemble_factor_of_one_member(so):
    torch, dev = _torch()
    c = _case(so, "rowmajor")
    f = c.g.lod_factor(c.mix[1].data_ptr(), c.cols.data_ptr())
    info = type(f.info)()
    c.g._check(c.g.lib.slod_lod_factor_get_info_member(f.f, 0, C.byref(info)))
    assert _same_words(info.min_pivot, f.info.min_pivot) and _same_words(info.max_pivot, f.info.max_pivot) and info.bytes == f.info.bytes
    B = _dev(np.random.default_rng(207).uniform(-1.0, 1.0, (c.nrow, 3)))
    X, Y = _nan(c.nrow, 3), _nan(c.nrow, 3)
    f.solve(B.data_ptr(), X.data_ptr(), n_rhs=3)
    c.g._check(c.g.lib.slod_lod_factor_solve_ensemble(f.f, 0, 1, B.data_ptr(), 3, 3, Y.data_ptr(), 3, None))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(X), _bits(Y))
    f.close()


# ---- one member that is not positive definite

def _lower_slot(c):
    """Word index of an entry strictly below the diagonal in factor order, in the middle of the band: block row of patch
    p, a slot whose column patch has a smaller cell index (cy N + cx), entry (0, 0)."""
    g = c.g
    cell = [g.patch_layout(p).cy * g.N + g.patch_layout(p).cx for p in range(c.NP)]
    p = cell.index(c.NP // 2)
    hc = c.hcols.reshape(c.NP, c.cap)
    j = [j for j in range(c.cap) if hc[p, j] != 0xffffffff and cell[int(hc[p, j])] < cell[p]][0]
    return (p * c.cap + j) * c.s * c.s


# A_1 - 1000 M_1 is indefinite where the lowest eigenvalue of the pencil (A_1, M_1) is below 1000: the two Poisson
# configurations.  For s2 (elasticity, D100 Lame fields) numpy.linalg.eigvalsh finds A_1 - 1000 M_1 positive definite
# (spectrum in [3.5, 340]), so there is nothing to refuse there; its NaN case runs.
BAD = [(name, what) for name in NAMES for what in ("indefinite", "NaN") if (name, what) != ("s2", "indefinite")]


@pytest.mark.parametrize("name,what", BAD)
def test_factor_ensemble_with_one_bad_member(so, name, what):
    import slod_amd
    torch, dev = _torch()
    c = _case(so, name)
    K = c.K
    if what == "indefinite":
        bad = _single_combine(c, 1.0, c.sym[1], -1000.0, c.mass[1])
        lam = np.linalg.eigvalsh(_dense(c, bad))
        assert lam[0] < 0.0 < lam[-1], (lam[0], lam[-1])
    else:
        bad = c.mix[1].clone()
        bad[_lower_slot(c)] = NAN
    # what the single call says of that matrix
    out = C.c_void_p(1)
    rc = c.g.lib.slod_lod_factor_create(c.g.h, bad.data_ptr(), c.cols.data_ptr(), C.byref(out))
    msg1 = c.g.lib.slod_last_error(c.g.h).decode()
    assert rc == -5 and out.value is None
    pivot = int(re.search(r"pivot (\d+) of", msg1).group(1))
    V = torch.stack([c.mix[0], bad, c.mix[2]], dim=1).contiguous()
    bp = (C.c_int32 * K)(7, 7, 7)
    out = C.c_void_p(1)
    rc = c.g.lib.slod_lod_factor_create_ensemble(c.g.h, V.data_ptr(), K, K, c.cols.data_ptr(), bp, C.byref(out))
    msg = c.g.lib.slod_last_error(c.g.h).decode()
    print("%s %s: single: %s; ensemble: %d, %s" % (name, what, msg1, rc, msg))
    assert rc == -5 and out.value is None
    assert list(bp) == [-1, pivot, -1]
    assert "slod_lod_factor_create_ensemble" in msg and "member 1" in msg and "pivot %d of" % pivot in msg
    with pytest.raises(slod_amd.SlodError) as e:
        c.g.lod_factor_ensemble(V.data_ptr(), c.cols.data_ptr(), K)
    assert e.value.code == -5 and e.value.bad_pivot.tolist() == [-1, pivot, -1]
    # the call without that member succeeds; its solves are those of the single factors
    keep = [k for k in range(K) if e.value.bad_pivot[k] < 0]
    assert keep == [0, 2]
    W = V[:, keep].contiguous()
    f = c.g.lod_factor_ensemble(W.data_ptr(), c.cols.data_ptr(), len(keep))
    B = _dev(np.random.default_rng(209).uniform(-1.0, 1.0, (c.nrow, len(keep))))
    X = _nan(c.nrow, len(keep))
    f.solve(B.data_ptr(), X.data_ptr())
    torch.cuda.synchronize()
    for i, k in enumerate(keep):
        (_, _, _, pmin, pmax), x = _single_factor_solve(c, c.mix[k], B, 1, first=i)
        assert np.array_equal(_bits(X[:, i]), _bits(x[:, 0])), (name, what, k)
        assert _same_words(f.member_info(i).min_pivot, pmin) and _same_words(f.member_info(i).max_pivot, pmax)
    f.close()


# ---- the theta scheme on an ensemble factor

def _stepper_members(c, K, dt, theta):
    """A_k, M_k, S_k = M_k + theta dt A_k interleaved [nval][K], S by the ensemble combination."""
    A, M = _stack(c, c.sym, K), _stack(c, c.mass, K)
    S = _nan(c.nval, K)
    c.g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), theta * dt, A.data_ptr(), K, S.data_ptr())
    return A, M, S


def _theta_model(A, M, dt, theta, n_steps, u, loads):
    S = M + theta * dt * A
    for k in range(n_steps):
        g = theta * loads(k + 1) + (1.0 - theta) * loads(k) - A @ u
        u = u + np.linalg.solve(S, dt * g)
    return u


@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("name", NAMES)
def test_theta_steps_ensemble_direct_equals_single_steppers(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    g, dt, steps, cols = c.g, 0.01, 3, c.cols.data_ptr()
    rng = np.random.default_rng(211)
    u0 = rng.uniform(-1.0, 1.0, (c.nrow, K))
    mscale = float(torch.stack(c.mass).abs().max())
    L = rng.uniform(-1.0, 1.0, (steps + 1, c.nrow, K)) * mscale
    Lt = _dev(L)
    worst = 0.0
    for theta in (1.0, 0.5):
        A, M, S = _stepper_members(c, K, dt, theta)
        f = g.lod_factor_ensemble(S.data_ptr(), cols, K)
        singles = []
        for k in range(K):
            Ak = A[:, k].contiguous()
            Sk = _single_combine(c, 1.0, M[:, k], theta * dt, Ak)
            assert np.array_equal(_bits(Sk), _bits(S[:, k]))
            singles.append((Ak, g.lod_factor(Sk.data_ptr(), cols)))
        for loading in ("none", "constant", "distinct"):
            load, stride, loads = {"none": (None, 0, lambda j: np.zeros((c.nrow, K))),
                                   "constant": (Lt[1], 0, lambda j: L[1]),
                                   "distinct": (Lt, c.nrow * K, lambda j: L[j])}[loading]
            Ue = _nan(c.nrow, K + 2)                                 # padded ld_u
            Ue[:, :K] = _dev(u0)
            g.lod_theta_steps_ensemble_direct(f, A.data_ptr(), cols, dt, theta, steps, K, Ue.data_ptr(), ld_u=K + 2,
                                              d_load=None if load is None else load.data_ptr(), load_step_stride=stride)
            assert torch.isnan(Ue[:, K:]).all() and torch.isfinite(Ue[:, :K]).all()
            for k in range(K):
                Ak, fk = singles[k]
                u = _dev(u0[:, k:k + 1])
                Lk = None if load is None else (Lt[:, :, k].contiguous() if loading == "distinct" else Lt[1, :, k].contiguous())
                g.lod_theta_steps_direct(fk, Ak.data_ptr(), cols, dt, theta, steps, u.data_ptr(),
                                         d_load=None if Lk is None else Lk.data_ptr(), load_step_stride=c.nrow if stride else 0)
                assert np.array_equal(_bits(Ue[:, k]), _bits(u[:, 0])), (name, K, theta, loading, k)
            if K == c.K:                                             # against the dense recursion per member
                hu = Ue[:, :K].cpu().numpy()
                for k in range(K):
                    ref = _theta_model(_dense(c, A[:, k]), _dense(c, M[:, k]), dt, theta, steps, u0[:, k],
                                       lambda j: loads(j)[:, k])
                    err = np.abs(hu[:, k] - ref).max() / np.abs(ref).max()
                    worst = max(worst, err)
                    assert err <= 1e-8, (name, theta, loading, k, err)
        # n_steps = 2 equals 2 x n_steps = 1, as words
        U2, U1 = _dev(u0), _dev(u0)
        g.lod_theta_steps_ensemble_direct(f, A.data_ptr(), cols, dt, theta, 2, K, U2.data_ptr(), d_load=Lt.data_ptr(),
                                          load_step_stride=c.nrow * K)
        for j in range(2):
            g.lod_theta_steps_ensemble_direct(f, A.data_ptr(), cols, dt, theta, 1, K, U1.data_ptr(), d_load=Lt[j].data_ptr(),
                                              load_step_stride=c.nrow * K)
        assert np.array_equal(_bits(U1), _bits(U2))
        for _, fk in singles:
            fk.close()
        f.close()
    if K == c.K:
        print("%s: theta steps on an ensemble factor, worst relative deviation from the dense recursion %.3e" % (name, worst))


def test_theta_steps_ensemble_direct_refuses_another_member_count(so):
    import slod_amd
    torch, dev = _torch()
    c = _case(so, "rowmajor")
    K, cols = c.K, c.cols.data_ptr()
    A, M, S = _stepper_members(c, K, 0.01, 1.0)
    f3 = c.g.lod_factor_ensemble(S.data_ptr(), cols, K)
    f1 = c.g.lod_factor(S[:, 0].contiguous().data_ptr(), cols)
    u = torch.zeros(c.nrow, K, dtype=torch.float64, device=dev)
    for call in (lambda: c.g.lod_theta_steps_ensemble_direct(f3, A.data_ptr(), cols, 0.01, 1.0, 1, K - 1, u.data_ptr(), ld_m=K, ld_u=K),
                 lambda: c.g.lod_theta_steps_ensemble_direct(f1, A.data_ptr(), cols, 0.01, 1.0, 1, K, u.data_ptr()),
                 lambda: c.g.lod_theta_steps_direct(f3, A[:, 0].contiguous().data_ptr(), cols, 0.01, 1.0, 1, u.data_ptr())):
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and "factor of another member count" in str(e.value)
    other = _case(so, "base")
    with pytest.raises(slod_amd.SlodError) as e:
        other.g.lod_theta_steps_ensemble_direct(f3, A.data_ptr(), cols, 0.01, 1.0, 1, K, u.data_ptr())
    assert e.value.code == -1 and "factor of another handle" in str(e.value)
    assert (u == 0.0).all()
    f1.close()
    f3.close()


# ---- end to end

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


def test_heat_pipeline_equals_three_single_pipelines(so):
    torch, dev = _torch()
    c = _case(so, "base")
    g, K, dt, steps = c.g, c.K, 0.01, 4
    V, M, A, S = _nan(c.nval, K), _nan(c.nval, K), _nan(c.nval, K), _nan(c.nval, K)
    cols, mcols = torch.zeros_like(c.cols), torch.zeros_like(c.cols)
    R, fine = _nan(c.nrow, K), _nan(K, c.field)
    Ut = torch.zeros(c.nrow, K, dtype=torch.float64, device=dev)
    mean, var = _nan(c.field), _nan(c.field)
    torch.cuda.synchronize()
    g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix_ensemble(c.b.data_ptr(), c.stride, K, M.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, A.data_ptr())
    g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), dt, A.data_ptr(), K, S.data_ptr())
    g.lod_rhs_ensemble(c.b.data_ptr(), c.stride, K, c.load.data_ptr(), R.data_ptr())
    f = g.lod_factor_ensemble(S.data_ptr(), cols.data_ptr(), K)
    g.lod_theta_steps_ensemble_direct(f, A.data_ptr(), cols.data_ptr(), dt, 1.0, steps, K, Ut.data_ptr(), d_load=R.data_ptr())
    g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, K, Ut.data_ptr(), fine.data_ptr())
    g.ensemble_moments(fine.data_ptr(), K, c.field, mean.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(cols, c.cols) and torch.equal(mcols, c.cols)
    single = []
    for k in range(K):
        Sk = _single_combine(c, 1.0, c.mass[k], dt, c.sym[k])
        fk = g.lod_factor(Sk.data_ptr(), c.cols.data_ptr())
        u = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
        g.lod_theta_steps_direct(fk, c.sym[k].data_ptr(), c.cols.data_ptr(), dt, 1.0, steps, u.data_ptr(), d_load=c.rhs[k].data_ptr())
        out = _nan(c.field)
        g.lod_reconstruct(c.slab[k][0].data_ptr(), c.stride, u.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Ut[:, k]), _bits(u[:, 0])), k
        single.append(out.cpu().numpy())
        fk.close()
    single = np.stack(single)
    assert np.array_equal(_bits(fine), single.view(np.uint64))
    m, v = _moments_numpy(single)
    assert np.array_equal(_bits(mean), m.view(np.uint64)) and np.array_equal(_bits(var), v.view(np.uint64))
    assert np.isfinite(single).all() and v.max() > 0.0 and np.abs(m).max() > 0.0
    f.close()


# ---- the driver

def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_driver_ensemble_heat_direct():
    """The smallest geometry of the driver tests (64 patches).  The last step's distances of member k are the L2 and
    energy lines of the table of a single --heat .. --direct run on member k's coefficient, to the digits printed."""
    K, steps = 3, 2
    out = _driver("--ensemble", str(K), "--heat", str(steps), "0.01", "--direct")
    lines = re.findall(r"^member (\d+) heat step (\d+): L2 distance = (\S+), energy distance = (\S+)$", out, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(k, j) for j in range(1, steps + 1) for k in range(K)], out
    dist = {(int(a), int(b)): (l2, en) for a, b, l2, en in lines}
    factor = re.findall(r"^factor: n = (\d+), half bandwidth = (\d+), bytes = (\d+), pivots in \[(\S+), (\S+)\]$", out, re.M)
    assert len(factor) == 2 and factor[0][:2] == factor[1][:2] == ("64", "27")          # member 0 alone, then the ensemble
    assert int(factor[1][2]) > (K - 1) * int(factor[0][2]) and float(factor[1][3]) > 0.0
    m = re.search(r"^SLOD heat ensemble of 3 at T = 0.02: L2 norm of the mean = (\S+), of the standard deviation = (\S+)$", out, re.M)
    assert m and float(m.group(1)) > 0.0 and float(m.group(2)) > 0.0, out
    for k in range(K):
        one = _driver("--member", str(k), "--heat", str(steps), "0.01", "--direct")
        table = one.split("vs elliptic SLOD solution")[1]
        rows = dict(re.findall(r"^  (\S+) +error = (\S+)", table, re.M))
        print("member %d: ensemble %s, single L2 %s energy %s" % (k, dist[(k, steps)], rows["L2"], rows["energy"]))
        assert dist[(k, steps)] == (rows["L2"], rows["energy"]), k
        for j in range(1, steps):                                    # the distance shrinks with every step
            assert float(dist[(k, j + 1)][0]) < float(dist[(k, j)][0])
    assert len({dist[(k, steps)] for k in range(K)}) == K            # the members differ
