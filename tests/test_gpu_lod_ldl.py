"""GPU tests of the banded LDL^T factor on the LOD space (slod_lod_factor_create_ldl, _create_ldl_ensemble,
slod_lod_factor_inertia) and of the consumers of a factor on it, against the unpivoted LDL^T in numpy of
lod_ldl_cases.py (checked on the CPU by test_lod_ldl_reference.py), scipy's spectrum, the Cholesky factor, and itself
as 64-bit words.

Cases: the four of test_gpu_lod_factor.py with their real sym(A) and M,
  dense     n = 16,  b = 15   one tile
  rowmajor  n = 25,  b = 18   padding in n and in b, row-major ids
  s2        n = 128, b = 55   elasticity
  morton16  n = 256, b = 51   16 block columns, Morton ids
each at five shifts sigma of S = sym(A) - sigma M: the rule shift_at of lod_ldl_cases.py at t = 1, rows / 4, rows / 2
(the first of eight gap midpoints with a relative gap >= 1e-6, the yardstick's inertia equal to scipy's count and the
yardstick's growth <= 1e4; none: the test fails), lambda_1 / 2 (no negative pivot) and 2 lambda_max (all negative).
The bars are those of lod_ldl_cases.py; the figures the tests print are recorded in DESIGN section 6.
"""
import ctypes as C
import re
import types

import numpy as np
import pytest

import lod_ldl_cases as lc
from lod_cases import NAN, _bits, _torch
from lod_eig_direct_cases import ensemble_case, same_words, shifted, stack

pytestmark = pytest.mark.gpu


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _solve(f, B, n, ld_u=None, first=0):
    """Out of place into a NaN-filled [nrow][ld_u]; columns first .. first + n of B."""
    torch, dev = _torch()
    ld_u = n if ld_u is None else ld_u
    out = torch.full((B.shape[0], ld_u), NAN, dtype=torch.float64, device=dev)
    f.solve(B.data_ptr() + 8 * first, out.data_ptr(), n_rhs=n, ld_rhs=B.shape[1], ld_u=ld_u)
    torch.cuda.synchronize()
    return out


def _combine(c, alpha, a, beta, b):
    torch, dev = _torch()
    out = torch.full_like(a, NAN)
    c.g.lod_matrix_combine(alpha, a.data_ptr(), beta, b.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def _dense(c, values):
    from lod_cases import _rows_to_dense
    return _rows_to_dense(c.g, values.cpu().numpy(), c.cols.cpu().numpy().view(np.uint32), c.s)


def _yardstick(c, S):
    return lc.ldl_reference(S[np.ix_(c.perm, c.perm)])


def _inertia_words(i):
    return (i.n_negative, i.n_positive, np.array([i.min_abs_pivot, i.max_abs_pivot, i.norm_matrix, i.norm_factor]).tobytes())


# ---- inertia, norms, backward error at the five shifts

@pytest.mark.parametrize("name", lc.CASES)
def test_ldl_inertia_norms_and_backward_error(so, name):
    c = lc.ldl_case(so, name)
    rng = np.random.default_rng(301)
    b = c.hbw
    for label, sigma, below, _ in c.shifts:
        values, S = lc.shifted_values(c, sigma)
        ref = _yardstick(c, S)                           # of the words the factor reads
        assert ref.bad < 0
        assert below == int((c.lam < sigma).sum())
        f = c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())
        info, ine = f.info, f.inertia()
        assert (info.n, info.half_bandwidth, info.block) == (c.nrow, b, 16)
        assert (ine.n_negative, ine.n_positive) == (below, c.nrow - below), (name, label, ine.n_negative, below)
        # get_info reports the signed range of D (a single pivot of an indefinite factor is not a stable quantity: only
        # the relations between the reported figures are asserted, the values are printed)
        assert (info.min_pivot < 0.0) == (below > 0) and (info.max_pivot > 0.0) == (below < c.nrow)
        assert ine.max_abs_pivot == max(abs(info.min_pivot), abs(info.max_pivot))
        assert 0.0 < ine.min_abs_pivot <= min(abs(info.min_pivot), abs(info.max_pivot))
        norm = float(np.abs(S).astype(np.longdouble).sum(axis=1).max())
        d_norm = abs(ine.norm_matrix - norm) / norm
        assert d_norm <= (2 * b + 2) * lc.U, (name, label, d_norm)
        d_G = abs(ine.norm_factor - ref.G) / ref.G
        assert 0.5 * ref.G <= ine.norm_factor <= 2.0 * ref.G, (name, label, ine.norm_factor, ref.G)
        worst, worst_fwd = 0.0, 0.0
        for n in (1, 3, 16, 17, 65):
            hb = rng.uniform(-1.0, 1.0, (c.nrow, n))
            x = _solve(f, _dev(hb), n).cpu().numpy()
            assert np.isfinite(x).all()
            e = lc.eta(S, ref.G, x, hb)
            sol = np.linalg.solve(S, hb)
            worst = max(worst, e.max())
            worst_fwd = max(worst_fwd, (np.abs(x - sol).max(axis=0) / np.abs(sol).max(axis=0)).max())
            assert (e <= lc.bound(b)).all(), (name, label, n, e.max(), lc.bound(b))
        print("%s %s: D in [%.3e, %.3e], yardstick [%.3e, %.3e]" % (name, label, info.min_pivot, info.max_pivot, ref.d.min(), ref.d.max()))
        print("%s %s: sigma %.6e, n_negative %d, growth %.3e (yardstick %.3e, norm_factor off by %.2e relative, norm_matrix by "
              "%.2e), backward error %.3e (bound %.3e), forward error %.3e"
              % (name, label, sigma, ine.n_negative, ine.growth, ref.G / ref.norm, d_G, d_norm, worst, lc.bound(b), worst_fwd))
        f.close()


# ---- definite input: against the Cholesky factor, and the theta stepper on an LDL^T factor

@pytest.mark.parametrize("name", lc.CASES)
def test_ldl_of_a_definite_matrix_agrees_with_cholesky(so, name):
    c = lc.ldl_case(so, name)
    rng = np.random.default_rng(303)
    mix = _combine(c, 1.0, c.mvalues, 0.01, c.sym)
    for label, values, A in (("sym(A)", c.sym, c.A), ("M + 0.01 A", mix, _dense(c, mix))):
        ref = _yardstick(c, A)
        fl = c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())
        fc = c.g.lod_factor(values.data_ptr(), c.cols.data_ptr())
        ine = fl.inertia()
        assert (ine.n_negative, ine.n_positive) == (0, c.nrow)
        # D of LDL^T is the squared diagonal of the Cholesky factor
        assert fl.info.min_pivot == pytest.approx(fc.info.min_pivot, rel=1e-10)
        assert fl.info.max_pivot == pytest.approx(fc.info.max_pivot, rel=1e-10)
        hb = rng.uniform(-1.0, 1.0, (c.nrow, 17))
        xl, xc = _solve(fl, _dev(hb), 17).cpu().numpy(), _solve(fc, _dev(hb), 17).cpu().numpy()
        el, ec = lc.eta(A, ref.G, xl, hb), lc.eta(A, ref.G, xc, hb)
        assert (el <= lc.bound(c.hbw)).all() and (ec <= lc.bound(c.hbw)).all(), (name, label, el.max(), ec.max())
        # A (xl - xc) is the difference of two residuals, each within the bound of its own solve
        gap = np.abs(A.astype(np.longdouble) @ (xl.astype(np.longdouble) - xc)).max(axis=0)
        room = lc.bound(c.hbw) * (ref.G * (np.abs(xl).max(axis=0) + np.abs(xc).max(axis=0)) + 2 * np.abs(hb).max(axis=0))
        assert (gap <= room).all(), (name, label, (gap / room).max())
        fwd = (np.abs(xl - xc).max(axis=0) / np.abs(xc).max(axis=0)).max()
        print("%s %s: growth %.3e, backward error LDL^T %.3e, Cholesky %.3e (bound %.3e), LDL^T against Cholesky %.3e"
              % (name, label, ine.growth, el.max(), ec.max(), lc.bound(c.hbw), fwd))
        fl.close()
        fc.close()


@pytest.mark.parametrize("name", ["morton16", "s2"])
def test_theta_steps_on_an_ldl_factor(so, name):
    c = lc.ldl_case(so, name)
    g, dt, steps, theta = c.g, 0.01, 3, 0.5
    S = _combine(c, 1.0, c.mvalues, theta * dt, c.sym)
    fl = g.lod_factor_ldl(S.data_ptr(), c.cols.data_ptr())
    fc = g.lod_factor(S.data_ptr(), c.cols.data_ptr())
    assert fl.inertia().n_negative == 0
    rng = np.random.default_rng(307)
    for n in (1, 3):
        u0 = rng.uniform(-1.0, 1.0, (c.nrow, n))
        L = _dev(rng.uniform(-1.0, 1.0, (steps + 1, c.nrow, n)) * np.abs(c.M).max())
        Ul, Uc = _dev(u0), _dev(u0)
        for f, Ux in ((fl, Ul), (fc, Uc)):
            g.lod_theta_steps_direct(f, c.sym.data_ptr(), c.cols.data_ptr(), dt, theta, steps, Ux.data_ptr(), n_rhs=n,
                                     d_load=L.data_ptr(), load_step_stride=c.nrow * n)
        got, ref = Ul.cpu().numpy(), Uc.cpu().numpy()
        rel = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s theta = 1/2, %d steps, n_rhs %d: LDL^T against Cholesky %.3e" % (name, steps, n, rel))
        assert np.isfinite(got).all() and rel <= 1e-8, (name, n, rel)
    fl.close()
    fc.close()


# ---- words, at an interior shift

@pytest.mark.parametrize("name", ["rowmajor", "morton16"])
def test_ldl_solve_bits(so, name):
    torch, dev = _torch()
    c = lc.ldl_case(so, name)
    label, sigma, below, _ = c.shifts[1]                 # t = rows / 4
    values, S = lc.shifted_values(c, sigma)
    ref_f = _yardstick(c, S)
    f = c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())
    assert 0 < f.inertia().n_negative == below < c.nrow
    K = 65
    hb = np.random.default_rng(311).uniform(-1.0, 1.0, (c.nrow, K))
    B = _dev(hb)
    wide = _solve(f, B, K)
    ref = _bits(wide)
    assert (lc.eta(S, ref_f.G, wide.cpu().numpy(), hb) <= lc.bound(c.hbw)).all()
    # a repeated solve
    assert np.array_equal(_bits(_solve(f, B, K)), ref)
    # a column as its own n_rhs = 1 run, ld = K
    for k in (0, 2, 15, 16, 63, 64):
        one = _solve(f, B, 1, first=k)
        assert np.array_equal(_bits(one[:, 0]), ref[:, k]), k
    # permuted columns
    perm = np.random.default_rng(313).permutation(K)
    got = _solve(f, B[:, torch.from_numpy(perm).to(dev)].contiguous(), K)
    assert np.array_equal(_bits(got), ref[:, perm])
    # padded ld_rhs / ld_u, NaN padding left untouched
    Bw = torch.full((c.nrow, K + 5), NAN, dtype=torch.float64, device=dev)
    Bw[:, :K] = B
    got = _solve(f, Bw, K, ld_u=K + 7)
    assert np.array_equal(_bits(got[:, :K]), ref) and bool(torch.isnan(got[:, K:]).all()) and bool(torch.isnan(Bw[:, K:]).all())
    # in place
    for n in (1, 17, K):
        X = B[:, :n].clone()
        f.solve(X.data_ptr(), X.data_ptr(), n_rhs=n)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(X), ref[:, :n]), n
    # a second factor of the same matrix
    f2 = c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())
    assert np.array_equal(_bits(_solve(f2, B, K)), ref)
    assert _inertia_words(f.inertia()) == _inertia_words(f2.inertia())
    assert np.array([f.info.min_pivot, f.info.max_pivot]).tobytes() == np.array([f2.info.min_pivot, f2.info.max_pivot]).tobytes()
    f2.close()
    f.close()


# ---- failure

def test_ldl_refuses_a_zero_pivot_and_nan(so):
    import slod_amd
    c = lc.ldl_case(so, "morton16")
    label, sigma, below, _ = c.shifts[2]
    good, S = lc.shifted_values(c, sigma)
    zeroed = good.clone()
    zeroed[lc.diagonal_word(c, 0)] = 0.0
    holed = good.clone()
    cap = c.g.lod_row_capacity()
    hc = c.cols.cpu().numpy().view(np.uint32).reshape(-1, cap)
    r = int(c.perm[c.nrow // 2])                       # a row in the middle of the band, s = 1: row = patch
    at = {int(row): k for k, row in enumerate(c.perm)}
    under = [j for j in range(cap) if hc[r, j] != 0xffffffff and at[int(hc[r, j])] < c.nrow // 2]
    holed[r * cap + under[0]] = NAN                    # an entry of the lower triangle in factor order
    Sh = S.copy()
    Sh[r, int(hc[r, under[0]])] = NAN                  # the yardstick reads the lower triangle in factor order only
    want = {"zero": 0, "NaN": lc.ldl_reference(Sh[np.ix_(c.perm, c.perm)]).bad}
    assert want["NaN"] == c.nrow // 2
    for what, values in (("zero", zeroed), ("NaN", holed)):
        out = C.c_void_p(1)
        rc = c.g.lib.slod_lod_factor_create_ldl(c.g.h, values.data_ptr(), c.cols.data_ptr(), C.byref(out))
        msg = c.g.lib.slod_last_error(c.g.h).decode()
        print("%s: %d, %s" % (what, rc, msg))
        assert rc == -5 and out.value is None and "slod_lod_factor_create_ldl:" in msg
        m = re.search(r"pivot (\d+) of %d is zero or not finite" % c.nrow, msg)
        assert m and int(m.group(1)) == want[what], (what, msg)
        with pytest.raises(slod_amd.SlodError) as e:
            c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())
        assert e.value.code == -5
        # after the failure a good factor passes the bound
        f = c.g.lod_factor_ldl(good.data_ptr(), c.cols.data_ptr())
        assert f.inertia().n_negative == below
        hb = np.random.default_rng(317).uniform(-1.0, 1.0, (c.nrow, 3))
        ref = _yardstick(c, S)
        assert (lc.eta(S, ref.G, _solve(f, _dev(hb), 3).cpu().numpy(), hb) <= lc.bound(c.hbw)).all()
        f.close()
    # a Cholesky factor has no inertia; a member out of range
    fc = c.g.lod_factor(c.sym.data_ptr(), c.cols.data_ptr())
    with pytest.raises(slod_amd.SlodError) as e:
        fc.inertia()
    assert e.value.code == -1 and "slod_lod_factor_inertia:" in str(e.value) and "Cholesky" in str(e.value)
    fc.close()
    f = c.g.lod_factor_ldl(good.data_ptr(), c.cols.data_ptr())
    for member in (-1, 1):
        with pytest.raises(slod_amd.SlodError) as e:
            f.inertia(member)
        assert e.value.code == -1 and "member" in str(e.value)
    f.close()


# ---- ensemble: every member has the words of the single call on its de-interleaved matrix

@pytest.mark.parametrize("name,K", [("base", 3), ("s2", 3), ("rowmajor", 3), ("base", 65)])
def test_ldl_ensemble_members_have_the_words_of_the_single_factor(so, name, K):
    import scipy.linalg as sl
    import slod_amd
    torch, dev = _torch()
    c = ensemble_case(so, name)
    g, cols = c.g, c.cols
    p = types.SimpleNamespace(g=g, s=c.s, nrow=c.nrow, cols=cols)   # what factor_order and diagonal_word read
    p.perm = lc.factor_order(p)
    lam = sl.eigh(c.A[0], c.M[0], eigvals_only=True)
    sigma = lc.shift_at(lam, c.A[0], c.M[0], c.nrow // 4, p.perm)[0]   # of member 0, one shift for all members
    V = stack(c, [shifted(g, cols, c.sym[k], c.mass[k], sigma) for k in range(c.K)], K, pad=2)
    f = g.lod_factor_ldl_ensemble(V.data_ptr(), cols.data_ptr(), K, ld_m=K + 2)
    assert (f.bad_pivot == -1).all()
    rng = np.random.default_rng(331)
    n_wide = 17
    hb = rng.uniform(-1.0, 1.0, (c.nrow, K * n_wide))
    B = _dev(hb)
    got = {}
    for n in (1, n_wide):
        Bn = B[:, :K * n].contiguous()
        out = torch.full((c.nrow, K * n), NAN, dtype=torch.float64, device=dev)
        f.solve(Bn.data_ptr(), out.data_ptr(), n_rhs=n)
        torch.cuda.synchronize()
        got[n] = (Bn, _bits(out))
    first, count = 1, min(K - 1, 2)                      # a member sub-range, 3 columns each
    Bs = B[:, :count * 3].contiguous()
    sub = torch.full((c.nrow, count * 3), NAN, dtype=torch.float64, device=dev)
    f.solve(Bs.data_ptr(), sub.data_ptr(), n_rhs=3, first_member=first, n_members=count)
    torch.cuda.synchronize()
    sub = _bits(sub)
    below = set()
    for k in range(K):
        Vk = V[:, k].contiguous()
        fk = g.lod_factor_ldl(Vk.data_ptr(), cols.data_ptr())
        mi, si = f.member_info(k), fk.info
        assert np.array([mi.min_pivot, mi.max_pivot]).tobytes() == np.array([si.min_pivot, si.max_pivot]).tobytes(), k
        assert _inertia_words(f.inertia(k)) == _inertia_words(fk.inertia()), k
        below.add(fk.inertia().n_negative)
        for n in (1, n_wide):
            Bn, words = got[n]
            one = _solve(fk, Bn[:, k * n:(k + 1) * n].contiguous(), n)
            assert np.array_equal(_bits(one), words[:, k * n:(k + 1) * n]), (k, n)
        if first <= k < first + count:
            j = k - first
            one = _solve(fk, Bs[:, j * 3:(j + 1) * 3].contiguous(), 3)
            assert np.array_equal(_bits(one), sub[:, j * 3:(j + 1) * 3]), k
        fk.close()
    print("%s K = %d: sigma %.6e, n_negative of the members %s" % (name, K, sigma, sorted(below)))
    f.close()
    # one member's (0, 0) in factor order zeroed: that member fails alone, and the call without it succeeds
    victim = 1
    W = V.clone()
    W[lc.diagonal_word(p, 0), victim] = 0.0
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_ldl_ensemble(W.data_ptr(), cols.data_ptr(), K, ld_m=K + 2)
    want = np.full(K, -1, dtype=np.int32)
    want[victim] = 0
    assert e.value.code == -5 and np.array_equal(e.value.bad_pivot, want), e.value.bad_pivot
    assert "slod_lod_factor_create_ldl_ensemble: member %d: pivot 0 of %d is zero or not finite" % (victim, c.nrow) in str(e.value)
    keep = [k for k in range(K) if k != victim]
    Wk = W[:, torch.tensor(keep, device=dev)].contiguous()
    f = g.lod_factor_ldl_ensemble(Wk.data_ptr(), cols.data_ptr(), K - 1)
    assert (f.bad_pivot == -1).all()
    f.close()
