"""CG on the LOD space preconditioned by a banded factor (slod_lod_solve_multi_precond, slod_lod_solve_ensemble_precond) on
the GPU, against the dense float64 yardstick of lod_pcg_cases.py on the matrices read back from the device.

Iteration bracket: at rel_tol = TAU the device's iterations[c] lies between the yardstick's count at 10 TAU and its count
at TAU / 10; before that is asserted the yardstick's own two counts must differ by at most 3 (lod_pcg_cases.check_bracket).
Solutions: 1e-8 of max |dense solve|, the project's bar for LOD-space solves.  True residuals: 10 max(TAU, the yardstick's).
Everything said to be equal is compared as 64-bit words.

Configurations: base (64 rows, truncated band), s2 (elasticity, 128 rows), rowmajor (25 rows, padding in n and b) of
lod_eig_direct_cases.py with the members const / D100 / D1e4, and the step64 change of the refresh tests (one fine element
of cell (3, 3) scaled by 1.5: 9 dirty patches of 64)."""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_eig_direct_cases as ec
import lod_ldl_cases as lc
import lod_pcg_cases as pc
from conftest import make_fields
from lod_cases import NAN, PENCIL_CONFIGS, _bits, _build, _lod_matrix, _rows_to_dense, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
TAU = 1e-10
BAR = 1e-8
MEMBER = 1          # D100: the member the single-matrix tests run on
_rhs = {}


def _loads(nrow, n=17):
    """[nrow][n] uniform in (-1, 1), one fixed array per row count"""
    if nrow not in _rhs:
        _rhs[nrow] = np.random.default_rng(4100 + nrow).uniform(-1.0, 1.0, (nrow, 17))
    return _rhs[nrow][:, :n]


def _multi(g, f, values, cols, B, ld_rhs=None, ld_u=None, tol=TAU, max_it=200, first=0, wide=None):
    """slod_lod_solve_multi_precond on NaN-padded arrays: (iterations, residuals, u [nrow][n], SlodError or None).
    wide: the n columns sit at column `first` of arrays [nrow][wide]."""
    import slod_amd
    torch, dev = _torch()
    nrow, n = B.shape
    ld_rhs, ld_u = wide or ld_rhs or n, wide or ld_u or n
    rhs, u = ec._nan(nrow, ld_rhs), ec._nan(nrow, ld_u)
    rhs[:, first:first + n] = ec._dev(B)
    torch.cuda.synchronize()
    err = None
    try:
        its, res = g.lod_solve_multi_precond(f, values.data_ptr(), cols.data_ptr(), rhs.data_ptr() + 8 * first, ld_rhs, n,
                                             u.data_ptr() + 8 * first, ld_u, tol, max_it)
    except slod_amd.SlodError as e:
        err, its, res = e, e.iterations, e.rel_residual
    torch.cuda.synchronize()
    keep = np.ones(ld_u, dtype=bool)
    keep[first:first + n] = False
    assert torch.isnan(u[:, keep]).all() and torch.isnan(rhs[:, first + n:]).all() and torch.isnan(rhs[:, :first]).all()  # padding
    return its.copy(), res.copy(), u[:, first:first + n].contiguous(), err


def _ensemble(g, f, V, cols, B, K, ld_m=None, ld=None, tol=TAU, max_it=200):
    """slod_lod_solve_ensemble_precond: (iterations, residuals, u [nrow][K], SlodError or None)"""
    import slod_amd
    torch, dev = _torch()
    nrow = B.shape[0]
    ld = ld or K
    rhs, u = ec._nan(nrow, ld), ec._nan(nrow, ld)
    rhs[:, :K] = ec._dev(B)
    torch.cuda.synchronize()
    err = None
    try:
        its, res = g.lod_solve_ensemble_precond(f, V.data_ptr(), cols.data_ptr(), rhs.data_ptr(), u.data_ptr(), K,
                                                ld_m=V.shape[1] if ld_m is None else ld_m, ld_rhs=ld, ld_u=ld, rel_tol=tol,
                                                max_iterations=max_it)
    except slod_amd.SlodError as e:
        err, its, res = e, e.iterations, e.rel_residual
    torch.cuda.synchronize()
    assert torch.isnan(u[:, K:]).all()
    return its.copy(), res.copy(), u[:, :K].contiguous(), err


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_columns(label, A, solve_P, B, its, u, expect=None):
    """every column: the bracket, the solution bar, the true residual.  Returns the largest solution error / max |x|."""
    U = u.cpu().numpy()
    worst = 0.0
    for c in range(B.shape[1]):
        b = B[:, c]
        lo, hi, ref_res = pc.bracket(A, solve_P, b, TAU)
        if expect is not None:
            assert (lo, hi) == (expect, expect), (label, c, lo, hi)
        x = np.linalg.solve(A, b)
        err = np.abs(U[:, c] - x).max() / np.abs(x).max()
        res = np.linalg.norm(b - A @ U[:, c]) / np.linalg.norm(b)
        print("%s column %d: %d iterations (reference %d .. %d), error %.2e, true residual %.2e (reference %.2e)"
              % (label, c, its[c], lo, hi, err, res, ref_res))
        pc.check_bracket("%s column %d" % (label, c), its[c], lo, hi)
        assert err <= BAR, (label, c, err)
        assert res <= 10.0 * max(TAU, ref_res), (label, c, res, ref_res)
        worst = max(worst, err)
    return worst


def _matrix(c, kind, k=MEMBER):
    """(device block rows, dense copy) of sym(A), M or M + 0.01 A of member k"""
    torch, dev = _torch()
    if kind == "A":
        return c.sym[k], c.A[k]
    if kind == "M":
        return c.mass[k], c.M[k]
    out = torch.full_like(c.sym[k], NAN)
    torch.cuda.synchronize()
    c.g.lod_matrix_combine(1.0, c.mass[k].data_ptr(), 0.01, c.sym[k].data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out, ec.dense(c, out)


class _Perm:
    """what lod_ldl_cases.diagonal_word reads of a case"""

    def __init__(self, c):
        self.g, self.s, self.cols, self.nrow = c.g, c.s, c.cols, c.nrow
        self.perm = lc.factor_order(self)


def _doubled(c, r, seed=5):
    """sym(A) of member MEMBER with r diagonal words doubled: (device values, dense copy, the words)"""
    torch, dev = _torch()
    w = _Perm(c)
    rows = np.random.default_rng(seed).choice(c.nrow, r, replace=False)
    words = [lc.diagonal_word(w, int(i)) for i in rows]
    v = c.sym[MEMBER].clone()
    for t in words:
        v[t] *= 2.0
    torch.cuda.synchronize()
    return v, ec.dense(c, v), words


# ---- 1. a factor on its own matrix

@pytest.mark.parametrize("kind", ["A", "M", "M+0.01A"])
@pytest.mark.parametrize("name", ec.NAMES)
def test_factor_on_its_own_matrix(so, name, kind):
    c = ec.ensemble_case(so, name)
    values, A = _matrix(c, kind)
    f = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
    solve = pc.dense_solver(A)
    for n in (1, 3, 17):
        B = _loads(c.nrow, n)
        its, res, u, err = _multi(c.g, f, values, c.cols, B)
        assert err is None
        worst = _check_columns("%s %s n_rhs %d" % (name, kind, n), A, solve, B, its, u, expect=1)
        assert (res <= TAU).all()
        print("%s %s n_rhs %d: worst error %.2e of max |x|" % (name, kind, n, worst))
    f.close()


# ---- 2. the rank bound

@pytest.mark.parametrize("r", [1, 3, 8])
def test_rank_bound(so, r):
    torch, dev = _torch()
    c = ec.ensemble_case(so, "base")
    values, A2, words = _doubled(c, r)
    A = c.A[MEMBER]
    assert np.linalg.matrix_rank(A2 - A) == r
    f = c.g.lod_factor(c.sym[MEMBER].data_ptr(), c.cols.data_ptr())        # of the unmodified matrix
    B = _loads(c.nrow, 3)
    solve = pc.dense_solver(A)
    for col in range(3):
        _, count, hist = pc.pcg_reference(A2, solve, B[:, col], TAU, 200)
        assert count <= r + 1, (r, col, count, hist)
        _, jac, _ = pc.jacobi_reference(A2, B[:, col], TAU, 5000)
        assert jac > r + 2, (r, col, jac)                                  # a condition on the input
    its, res, u, err = _multi(c.g, f, values, c.cols, B)
    assert err is None
    _check_columns("rank %d" % r, A2, solve, B, its, u)
    # Jacobi-CG of slod_lod_solve_multi on the same system
    rhs, uj = ec._dev(B), ec._nan(c.nrow, 3)
    torch.cuda.synchronize()
    jits, _ = c.g.lod_solve_multi(values.data_ptr(), c.cols.data_ptr(), rhs.data_ptr(), 3, 3, uj.data_ptr(), 3, TAU, 5000)
    print("rank %d: iterations %s with the stale factor, %s with Jacobi" % (r, list(its), list(jits)))
    assert (its < jits).all()
    f.close()


# ---- 3. the refresh pipeline

def test_refresh_pipeline_with_the_stale_factor(so):
    torch, dev = _torch()
    c = _build(so, PENCIL_CONFIGS["step64"])
    g, NP, cols = c.g, c.g.num_patches, c.cols
    NE = g.NE

    def sym(v):
        out = torch.full_like(v, NAN)
        torch.cuda.synchronize()
        g.lod_matrix_symmetrize(v.data_ptr(), cols.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        return out

    f_old = g.lod_factor(sym(c.values).data_ptr(), cols.data_ptr())
    # the change of the refresh tests: fine element (7, 6) times 1.5
    cfg = so.make_cfg(stabilize=1, **PENCIL_CONFIGS["step64"])
    new = [a.copy() for a in make_fields(so, cfg, "D100")]
    new[0][(6 * NE + 7) * 4:(6 * NE + 7) * 4 + 4] *= 1.5
    dirty = torch.zeros(NP, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.update_coefficient(0, new[0], dirty.data_ptr())
    n_dirty = len(g.dirty_patches(dirty.data_ptr()))
    assert n_dirty == 9
    plan = g.plan_dirty(dirty.data_ptr())
    b1, q1, A1 = c.b.clone(), c.q.clone(), c.values.clone()
    torch.cuda.synchronize()
    plan.execute(b1.data_ptr(), q1.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    g.lod_matrix_update(dirty.data_ptr(), b1.data_ptr(), q1.data_ptr(), c.stride, A1.data_ptr())
    torch.cuda.synchronize()
    S1 = sym(A1)
    load = torch.zeros((NE + 1) ** 2, dtype=torch.float64, device=dev)
    rhs = ec._nan(NP)
    torch.cuda.synchronize()
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()
    g.lod_rhs(np.arange(NP), b1.data_ptr(), c.stride, load.data_ptr(), rhs.data_ptr())
    torch.cuda.synchronize()
    B = rhs.cpu().numpy().reshape(NP, 1)
    A_new = _rows_to_dense(g, S1.cpu().numpy(), cols.cpu().numpy().view(np.uint32), 1)
    A_old = _rows_to_dense(g, sym(c.values).cpu().numpy(), cols.cpu().numpy().view(np.uint32), 1)
    its, res, u, err = _multi(g, f_old, S1, cols, B)
    assert err is None
    _check_columns("refresh, %d dirty" % n_dirty, A_new, pc.dense_solver(A_old), B, its, u)
    assert its[0] >= 2
    x = np.linalg.solve(A_new, B[:, 0])
    # the stale factor alone is further from the solution: the iteration did the work
    stale = ec._nan(NP)
    torch.cuda.synchronize()
    f_old.solve(rhs.data_ptr(), stale.data_ptr())
    torch.cuda.synchronize()
    e_pcg, e_stale = np.abs(u.cpu().numpy()[:, 0] - x).max(), np.abs(stale.cpu().numpy() - x).max()
    print("refresh: %d iterations, error %.2e with PCG, %.2e with the stale factor alone" % (its[0], e_pcg, e_stale))
    assert e_stale > 100.0 * e_pcg
    # the full rebuild on the changed coefficient: build, matrix, factor, solve, reconstruct
    plan_f = g.plan(np.arange(NP, dtype=np.uint32))
    bf, qf = torch.zeros_like(c.b), torch.zeros_like(c.q)
    torch.cuda.synchronize()
    plan_f.execute(bf.data_ptr(), qf.data_ptr())
    plan_f.status()
    torch.cuda.synchronize()
    Af, _ = _lod_matrix(g, bf, qf, c.stride, 1)
    f_new = g.lod_factor(sym(Af).data_ptr(), cols.data_ptr())
    rhs_f, u_f, fine_f, fine_1 = ec._nan(NP), ec._nan(NP), ec._nan((NE + 1) ** 2), ec._nan((NE + 1) ** 2)
    torch.cuda.synchronize()
    g.lod_rhs(np.arange(NP), bf.data_ptr(), c.stride, load.data_ptr(), rhs_f.data_ptr())
    f_new.solve(rhs_f.data_ptr(), u_f.data_ptr())
    torch.cuda.synchronize()
    g.lod_reconstruct(bf.data_ptr(), c.stride, u_f.data_ptr(), fine_f.data_ptr())
    g.lod_reconstruct(b1.data_ptr(), c.stride, u.data_ptr(), fine_1.data_ptr())
    torch.cuda.synchronize()
    d = (fine_1 - fine_f).abs().max().item() / fine_f.abs().max().item()
    print("refresh: reconstruction differs from the full rebuild by %.2e of its maximum" % d)
    assert d <= BAR
    f_old.close()
    f_new.close()
    g.close()


# ---- 4. ensembles

@pytest.mark.parametrize("name", ec.NAMES)
def test_ensemble_shared_and_per_member_factors(so, name):
    torch, dev = _torch()
    c = ec.ensemble_case(so, name)
    g, K = c.g, c.K
    V = ec.stack(c, c.sym, K)
    Vpad = ec.stack(c, c.sym, K, pad=2)
    # member 0 takes a general load; under member 0's factor the others take a load of five modes of (A_k, A_0), on which
    # the yardstick ends after five iterations and its counts at 10 TAU and TAU / 10 stay together (a general load needs
    # about 30 iterations on base and gains half a digit in each: 27 .. 32)
    B = np.stack([_loads(c.nrow, 1)[:, 0]] + [pc.few_mode_load(c.A[k], c.A[0]) for k in range(1, K)], axis=1)
    torch.cuda.synchronize()
    singles = [g.lod_factor(s.data_ptr(), c.cols.data_ptr()) for s in c.sym]
    shared = singles[0]
    its, res, u, err = _ensemble(g, shared, V, c.cols, B, K)
    assert err is None
    solve0 = pc.dense_solver(c.A[0])
    for k in range(K):
        _check_columns("%s shared, member %d" % (name, k), c.A[k], solve0, B[:, k:k + 1], its[k:k + 1], u[:, k:k + 1],
                       expect=1 if k == 0 else None)
        si, sr, su, _ = _multi(g, shared, c.sym[k], c.cols, B[:, k:k + 1])
        assert si[0] == its[k] and sr.view(np.uint64)[0] == res.view(np.uint64)[k] and _same(su[:, 0], u[:, k]), (name, k)
    # NaN-padded ld_m, ld_rhs, ld_u: the same words
    pits, pres, pu, _ = _ensemble(g, shared, Vpad, c.cols, B, K, ld=K + 3)
    assert torch.isnan(Vpad[:, K:]).all()
    assert np.array_equal(pits, its) and np.array_equal(pres.view(np.uint64), res.view(np.uint64)) and _same(pu, u)
    # a factor per member
    fe = g.lod_factor_ensemble(V.data_ptr(), c.cols.data_ptr(), K)
    its, res, u, err = _ensemble(g, fe, V, c.cols, B, K)
    assert err is None
    for k in range(K):
        _check_columns("%s per member, member %d" % (name, k), c.A[k], pc.dense_solver(c.A[k]), B[:, k:k + 1], its[k:k + 1],
                       u[:, k:k + 1], expect=1)
        si, sr, su, _ = _multi(g, singles[k], c.sym[k], c.cols, B[:, k:k + 1])
        assert si[0] == its[k] and sr.view(np.uint64)[0] == res.view(np.uint64)[k] and _same(su[:, 0], u[:, k]), (name, k)
    fe.close()
    for f in singles:
        f.close()


def test_ensemble_of_65_members_crosses_the_tiles(so):
    """K = 65 scaled copies on base: more than the 16 columns of a block of the factor solve and than LOD_COLS = 64"""
    torch, dev = _torch()
    c = ec.ensemble_case(so, "base")
    g, K = c.g, 65
    V = ec.stack(c, c.sym, K)
    B = np.tile(_loads(c.nrow, 13), (1, 5))
    torch.cuda.synchronize()
    shared = g.lod_factor(c.sym[0].data_ptr(), c.cols.data_ptr())
    fe = g.lod_factor_ensemble(V.data_ptr(), c.cols.data_ptr(), K)
    for label, f in (("shared", shared), ("per member", fe)):
        its, res, u, err = _ensemble(g, f, V, c.cols, B, K)
        assert err is None and (its >= 1).all() and (res <= TAU).all()
        if f is fe:
            assert (its == 1).all()
        for k in (0, 1, 15, 16, 17, 47, 63, 64):
            Ak = V[:, k].contiguous()
            torch.cuda.synchronize()
            fk = shared if f is shared else g.lod_factor(Ak.data_ptr(), c.cols.data_ptr())
            si, sr, su, _ = _multi(g, fk, Ak, c.cols, B[:, k:k + 1])
            assert si[0] == its[k] and sr.view(np.uint64)[0] == res.view(np.uint64)[k] and _same(su[:, 0], u[:, k]), (label, k)
            if fk is not shared:
                fk.close()
        print("65 members, %s factor: iterations %d .. %d" % (label, its.min(), its.max()))
    shared.close()
    fe.close()


# ---- 5. words

def test_words_do_not_depend_on_position_width_padding_or_run(so):
    torch, dev = _torch()
    c = ec.ensemble_case(so, "base")
    g = c.g
    values, A2, _ = _doubled(c, 3)                                          # a few iterations per column
    f = g.lod_factor(c.sym[MEMBER].data_ptr(), c.cols.data_ptr())
    B = _loads(c.nrow, 6).copy()
    B[:, 2] = 0.0                                                            # a zero column
    B[:, 4] *= 1e-3
    its, res, u, err = _multi(g, f, values, c.cols, B)
    assert err is None
    assert its[2] == 0 and res[2] == 0.0 and not _bits(u[:, 2]).any()       # exact zeros
    assert (np.delete(its, 2) >= 2).all()
    # a column equals its own n_rhs = 1 run
    for col in range(6):
        si, sr, su, _ = _multi(g, f, values, c.cols, B[:, col:col + 1])
        assert si[0] == its[col] and sr.view(np.uint64)[0] == res.view(np.uint64)[col] and _same(su[:, 0], u[:, col]), col
    # permuted columns
    perm = np.array([3, 5, 0, 2, 1, 4])
    pi, pr, pu, _ = _multi(g, f, values, c.cols, B[:, perm])
    assert np.array_equal(pi, its[perm]) and np.array_equal(pr.view(np.uint64), res.view(np.uint64)[perm]) and _same(pu, u[:, perm])
    # NaN-padded leading dimensions (the padding is checked in _multi), a column sub-range of a wider array, a repeated call
    for kw in (dict(ld_rhs=9, ld_u=7), dict(first=2, wide=11), dict()):
        qi, qr, qu, _ = _multi(g, f, values, c.cols, B, **kw)
        assert np.array_equal(qi, its) and np.array_equal(qr.view(np.uint64), res.view(np.uint64)) and _same(qu, u), kw
    # max_iterations = 0 and 1
    zi, zr, zu, _ = _multi(g, f, values, c.cols, B, max_it=0)
    assert not zi.any() and not _bits(zu).any() and np.array_equal(zr, np.where(np.arange(6) == 2, 0.0, 1.0))
    oi, orr, ou, _ = _multi(g, f, values, c.cols, B, max_it=1)
    assert np.array_equal(oi, np.where(np.arange(6) == 2, 0, 1)) and (np.delete(orr, 2) > TAU).all()
    for col in (0, 2, 5):
        si, sr, su, _ = _multi(g, f, values, c.cols, B[:, col:col + 1], max_it=1)
        assert si[0] == oi[col] and sr.view(np.uint64)[0] == orr.view(np.uint64)[col] and _same(su[:, 0], ou[:, col])
    # a cap inside the run: the counters stop at it, whatever the read-back interval
    cap = int(its.max()) - 1
    ci, cr, cu, _ = _multi(g, f, values, c.cols, B, max_it=cap)
    assert np.array_equal(ci, np.minimum(its, cap))
    f.close()


# ---- 6. the failure path

def test_breakdown_returns_numeric_and_leaves_handle_and_factor_usable(so):
    torch, dev = _torch()
    c = ec.ensemble_case(so, "base")
    g, K = c.g, c.K
    f = g.lod_factor(c.sym[MEMBER].data_ptr(), c.cols.data_ptr())
    B = _loads(c.nrow, 3)
    good = _multi(g, f, c.sym[MEMBER], c.cols, B)
    assert good[3] is None and (good[0] == 1).all()
    # - sym(A) with the factor of sym(A): p.Ap < 0 in the first iteration
    neg = -c.sym[MEMBER]
    its, res, u, err = _multi(g, f, neg, c.cols, B)
    assert err is not None and err.code == -5, err
    print(err)
    assert "slod_lod_solve_multi_precond: column 0, iteration 1: p.Ap = -" in str(err) and "is not > 0" in str(err)
    assert (its == 1).all() and not _bits(u).any()                           # frozen where it stood: u = 0
    # one NaN word in member 1 of an ensemble matrix
    w = _Perm(c)
    V = ec.stack(c, c.sym, K)
    V[lc.diagonal_word(w, 5), 1] = NAN
    fe = g.lod_factor_ensemble(ec.stack(c, c.sym, K).data_ptr(), c.cols.data_ptr(), K)
    its, res, u, err = _ensemble(g, fe, V, c.cols, B, K)
    assert err is not None and err.code == -5, err
    print(err)
    assert "slod_lod_solve_ensemble_precond: member 1, iteration 1: p.Ap = nan" in str(err)
    for k in (0, 2):
        fk = g.lod_factor(c.sym[k].data_ptr(), c.cols.data_ptr())
        si, sr, su, e1 = _multi(g, fk, c.sym[k], c.cols, B[:, k:k + 1])
        assert e1 is None and si[0] == its[k] == 1 and sr.view(np.uint64)[0] == res.view(np.uint64)[k] and _same(su[:, 0], u[:, k])
        fk.close()
    # the same handle and factor solve a good system, with the words of before
    again = _multi(g, f, c.sym[MEMBER], c.cols, B)
    assert again[3] is None and np.array_equal(again[0], good[0]) and _same(again[2], good[2])
    assert np.array_equal(again[1].view(np.uint64), good[1].view(np.uint64))
    fe.close()
    f.close()


# ---- 7. the kind of the preconditioner, and the refusals that need a factor

def test_preconditioner_kind_and_factor_refusals(so):
    import scipy.linalg as sl
    import slod_amd
    torch, dev = _torch()
    c = ec.ensemble_case(so, "base")
    g, K = c.g, c.K
    B = _loads(c.nrow, 3)
    f = g.lod_factor_ldl(c.sym[MEMBER].data_ptr(), c.cols.data_ptr())
    assert f.inertia().n_negative == 0
    its, res, u, err = _multi(g, f, c.sym[MEMBER], c.cols, B)
    assert err is None
    _check_columns("LDL^T of sym(A)", c.A[MEMBER], pc.dense_solver(c.A[MEMBER]), B, its, u, expect=1)
    f.close()
    lam = sl.eigh(c.A[MEMBER], c.M[MEMBER], eigvals_only=True)
    sigma = 0.5 * (lam[1] + lam[2])
    S = ec.shifted(g, c.cols, c.sym[MEMBER], c.mass[MEMBER], sigma)
    f = g.lod_factor_ldl(S.data_ptr(), c.cols.data_ptr())
    assert f.inertia().n_negative > 0
    its, res, u, err = _multi(g, f, c.sym[MEMBER], c.cols, B)
    assert err is not None and err.code == -1 and "the preconditioner must be positive definite" in str(err), err
    assert "slod_lod_solve_multi_precond:" in str(err) and torch.isnan(u).all()
    V = ec.stack(c, c.sym, K)
    its, res, u, err = _ensemble(g, f, V, c.cols, B, K)
    assert err is not None and err.code == -1 and "the preconditioner must be positive definite" in str(err), err
    f.close()
    # member counts: the multi call takes one member, the ensemble call one or n_members
    fe = g.lod_factor_ensemble(V.data_ptr(), c.cols.data_ptr(), K)
    _, _, _, err = _multi(g, fe, c.sym[MEMBER], c.cols, B)
    assert err.code == -1 and str(err).endswith("slod_lod_solve_multi_precond: factor of another member count"), err
    _, _, _, err = _ensemble(g, fe, V, c.cols, B[:, :2], 2)
    assert err.code == -1 and str(err).endswith("slod_lod_solve_ensemble_precond: factor of another member count"), err
    fe.close()
    # a factor of another handle
    other = ec.ensemble_case(so, "rowmajor")
    fo = other.g.lod_factor(other.sym[0].data_ptr(), other.cols.data_ptr())
    _, _, _, err = _multi(g, fo, c.sym[MEMBER], c.cols, B)
    assert err.code == -1 and "slod_lod_solve_multi_precond: factor of another handle / row count" in str(err), err
    fo.close()


# ---- 8. the driver

DRIVER = dict(nref=3, n_sub=4, oversampling=1, spacedim=1)       # bin/main_Diffusion 3 4 1 1 (stabilised)
DRIVER_TOL, DRIVER_MAX_IT = 1e-13, 5000                          # lod_rel_tol, lod_max_iterations of host/LOD.cc


def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _driver_fields(so, NE, K):
    """The driver's Alpha(1, 100, 3) under srand(1), then K - 1 further draws of the same rand() stream (host/Diffusion.h:
    the members of an ensemble are drawn after Alpha, without reseeding)."""
    fields = [so.fill_coefficient_rand(1.0, 100.0, 3, NE, seed=1)]
    for _ in range(1, K):
        out = np.empty(NE * NE * 4, dtype=np.float64)
        so.lib().so_fill_coefficient_rand(1.0, 100.0, 3, NE, so._dp(out))
        fields.append(out)
    return fields


def _flip_cells(field, NE, n_cells, lo=1.0, hi=100.0, r=3):
    """DiffusionProblem::flip_coefficient_cells (host/Diffusion.h) on a per-quadrature-point field: n_cells cells of the
    2^r x 2^r grid picked by the LCG state = state * 1664525 + 1013904223 from 12345, cell = (state >> 8) % total (x
    fastest), flip between the extremes."""
    side = 1 << r
    per = NE // side
    f = field.copy().reshape(NE, NE, 4)
    state = 12345
    for _ in range(n_cells):
        state = (state * 1664525 + 1013904223) & 0xffffffff
        cell = (state >> 8) % (side * side)
        cx, cy = cell % side, cell // side
        block = f[cy * per:(cy + 1) * per, cx * per:(cx + 1) * per, :]
        assert (block == block[0, 0, 0]).all()
        block[...] = hi if block[0, 0, 0] < 0.5 * (lo + hi) else lo
    return f.ravel()


def test_driver_reuse_factor_matches_the_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --perturb 1 --reuse-factor against the same steps through the Python wrappers on the
    driver's own coefficient: the dirty count, the PCG and the Jacobi-CG iterations are equal, max |u| to the digits
    printed; the distance to the rebuild is below the 1e-8 bar.  --perturb 1 alone prints what it printed before."""
    torch, dev = _torch()
    out = _driver("3", "4", "1", "1", "--perturb", "1", "--reuse-factor")
    print(out)
    m = re.search(r"^stale factor as preconditioner: dirty patches = (\d+) of (\d+), PCG iterations = (\d+), "
                  r"Jacobi-CG iterations = (\d+)$", out, re.M)
    assert m, out
    n_dirty, n_patches, pcg, jac = (int(x) for x in m.groups())
    d = re.search(r"max \|u_pcg - u_rebuild\| = (\S+) +\(max \|u_rebuild\| = (\S+)\)", out)
    assert d, out
    assert float(d.group(2)) > 0.0 and float(d.group(1)) <= BAR * float(d.group(2)), d.group(0)
    # without --reuse-factor the run prints what it printed before, and nothing of this
    plain = _driver("3", "4", "1", "1", "--perturb", "1")
    assert "stale factor" not in plain and "u_pcg" not in plain
    assert [l for l in out.splitlines() if "stale factor" not in l and "u_pcg" not in l and "time" not in l.lower()] \
        == [l for l in plain.splitlines() if "time" not in l.lower()]
    # the Python path: factor, update, dirty plan, matrix update, symmetrize, the two solves
    c = _build(so, DRIVER, fields=_driver_fields(so, (1 << DRIVER["nref"]) * DRIVER["n_sub"], 1))
    g, NP, cols = c.g, c.g.num_patches, c.cols
    NE = g.NE

    def sym(v):
        o = torch.full_like(v, NAN)
        torch.cuda.synchronize()
        g.lod_matrix_symmetrize(v.data_ptr(), cols.data_ptr(), o.data_ptr())
        torch.cuda.synchronize()
        return o

    f_old = g.lod_factor(sym(c.values).data_ptr(), cols.data_ptr())
    dirty = torch.zeros(NP, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.update_coefficient(0, _flip_cells(_driver_fields(so, NE, 1)[0], NE, 1), dirty.data_ptr())
    py_dirty = len(g.dirty_patches(dirty.data_ptr()))
    plan = g.plan_dirty(dirty.data_ptr())
    plan.execute(c.b.data_ptr(), c.q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    g.lod_matrix_update(dirty.data_ptr(), c.b.data_ptr(), c.q.data_ptr(), c.stride, c.values.data_ptr())
    torch.cuda.synchronize()
    S1 = sym(c.values)
    load = torch.zeros((NE + 1) ** 2, dtype=torch.float64, device=dev)
    rhs, u, uj = ec._nan(NP), ec._nan(NP), ec._nan(NP)
    torch.cuda.synchronize()
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()
    g.lod_rhs(np.arange(NP), c.b.data_ptr(), c.stride, load.data_ptr(), rhs.data_ptr())
    torch.cuda.synchronize()
    pits, _ = g.lod_solve_multi_precond(f_old, S1.data_ptr(), cols.data_ptr(), rhs.data_ptr(), 1, 1, u.data_ptr(), 1, DRIVER_TOL,
                                        DRIVER_MAX_IT)
    jits, _ = g.lod_solve_multi(S1.data_ptr(), cols.data_ptr(), rhs.data_ptr(), 1, 1, uj.data_ptr(), 1, DRIVER_TOL, DRIVER_MAX_IT)
    torch.cuda.synchronize()
    print("python path: dirty %d, PCG %d, Jacobi-CG %d, max |u| %.6e" % (py_dirty, pits[0], jits[0], u.abs().max().item()))
    assert (n_dirty, n_patches) == (py_dirty, NP)
    assert pcg == pits[0] and jac == jits[0], (pcg, pits, jac, jits)
    assert "%.6e" % u.abs().max().item() == d.group(2)
    f_old.close()
    g.close()


def test_driver_ensemble_precond_member_matches_the_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --ensemble 3 --precond-member 0 against the Python wrappers on the driver's three
    coefficient fields: per member the PCG iterations under member 0's factor and the iterations of
    slod_lod_solve_ensemble on the same symmetrised systems are equal."""
    import slod_amd
    torch, dev = _torch()
    K = 3
    out = _driver("3", "4", "1", "1", "--ensemble", str(K), "--precond-member", "0")
    print(out)
    rows = re.findall(r"^member (\d+): PCG iterations = (\d+), Jacobi-CG iterations = (\d+)$", out, re.M)
    assert [int(r[0]) for r in rows] == list(range(K)), out
    plain = _driver("3", "4", "1", "1", "--ensemble", str(K))
    assert "PCG iterations" not in plain
    assert [l for l in out.splitlines() if "PCG iterations" not in l and "time" not in l.lower()] \
        == [l for l in plain.splitlines() if "time" not in l.lower()]
    # the Python path: one plan over the three members, the ensemble matrix, its symmetrised form, the shared load
    g = slod_amd.Slod(nref=DRIVER["nref"], n_sub=DRIVER["n_sub"], oversampling=DRIVER["oversampling"], spacedim=1, n_problems=K)
    NP, cap, NE = g.num_patches, g.lod_row_capacity(), g.NE
    for k, field in enumerate(_driver_fields(so, NE, K)):
        g.set_coefficient(0, field, problem=k)
    plan = g.plan(np.arange(K * NP, dtype=np.uint32))
    b = torch.zeros(K * NP * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    torch.cuda.synchronize()
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    V, S = ec._nan(NP * cap, K), ec._nan(NP * cap, K)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    load = torch.zeros((NE + 1) ** 2, dtype=torch.float64, device=dev)
    rhs, u = ec._nan(NP, K), ec._nan(NP, K)
    torch.cuda.synchronize()
    g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), plan.stride, K, V.data_ptr(), cols.data_ptr())
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, S.data_ptr())
    g.lod_rhs_ensemble(b.data_ptr(), plan.stride, K, load.data_ptr(), rhs.data_ptr())
    torch.cuda.synchronize()
    f0 = g.lod_factor_ensemble(S.data_ptr(), cols.data_ptr(), 1, ld_m=K)          # member 0 inside the wider array
    pits, _ = g.lod_solve_ensemble_precond(f0, S.data_ptr(), cols.data_ptr(), rhs.data_ptr(), u.data_ptr(), K, rel_tol=DRIVER_TOL,
                                           max_iterations=DRIVER_MAX_IT)
    jits, _ = g.lod_solve_ensemble(S.data_ptr(), cols.data_ptr(), rhs.data_ptr(), u.data_ptr(), K, rel_tol=DRIVER_TOL,
                                   max_iterations=DRIVER_MAX_IT)
    print("python path: PCG %s, Jacobi-CG %s" % (list(pits), list(jits)))
    assert pits[0] == 1                                                      # member 0 under its own factor
    assert [int(r[1]) for r in rows] == list(pits) and [int(r[2]) for r in rows] == list(jits), (rows, pits, jits)
    f0.close()
    g.close()
