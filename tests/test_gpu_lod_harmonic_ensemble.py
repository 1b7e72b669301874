"""GPU tests of the frequency response of a coefficient ensemble on the LOD space: slod_lod_factor_create_zldl_ensemble,
slod_lod_factor_solve_complex_ensemble and slod_lod_harmonic_response_ensemble, against the numpy yardstick and the modal
response of lod_harmonic_cases.py (checked on the CPU by test_lod_harmonic_ensemble_reference.py), numpy.linalg.solve, and
the single calls slod_lod_factor_create_zldl / slod_lod_harmonic_response on every member's own matrices as 64-bit words.

Cases: base (64 rows, truncated band), s2 (elasticity, 128 rows) and rowmajor (25 rows, padding in n and b) of
lod_eig_direct_cases.ensemble_case, members const / D100 / D1e4, at the ten frequencies of the ensemble sweep rule and
the three dampings of lod_harmonic_ensemble_cases.py; the growth cap is asserted on the yardstick of every member before
the library is called.  The layout, the rule and the bars are stated in lod_harmonic_ensemble_cases.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lod_harmonic_cases as hc
import lod_harmonic_ensemble_cases as he
from lod_cases import NAN, _bits, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _nan(rows, ld):
    torch, dev = _torch()
    return torch.full((rows, ld), NAN, dtype=torch.float64, device=dev)


def _ptr(t, first=0):
    return None if t is None else t.data_ptr() + 8 * first


def _z(ur, ui):
    return ur.cpu().numpy() + 1j * ui.cpu().numpy()


def _words(ur, ui):
    return np.stack([_bits(ur), _bits(ui)])


def _info_words(f, k):
    i, m = f.inertia(k), f.member_info(k)
    assert (i.n_negative, i.n_positive) == (-1, -1)
    return np.array([i.min_abs_pivot, i.max_abs_pivot, i.norm_matrix, i.norm_factor, m.min_pivot, m.max_pivot]).tobytes()


def _loads(rng, rows, n, complex_load=True):
    hr = rng.uniform(-1.0, 1.0, (rows, n))
    hi = rng.uniform(-1.0, 1.0, (rows, n)) if complex_load else np.zeros((rows, n))
    return hr + 1j * hi, _dev(hr), _dev(hi) if complex_load else None


def _padded(t, pad):
    """t with `pad` NaN columns behind it."""
    out = _nan(t.shape[0], t.shape[1] + pad)
    out[:, :t.shape[1]] = t
    return out


def _ensemble_factor(c, alpha, beta, K=None, pads=(2, 5)):
    """The factor on the NaN-padded ensemble matrices, ld_a_m = K + 2 and ld_b_m = K + 5."""
    K = c.K if K is None else K
    A, M = he.stack(c, c.sym, K, pad=pads[0]), he.stack(c, c.mass, K, pad=pads[1])
    f = c.g.lod_factor_zldl_ensemble(A.data_ptr(), M.data_ptr(), c.cols.data_ptr(), K, alpha, beta, ld_a_m=K + pads[0],
                                     ld_b_m=K + pads[1])
    return f, A, M


def _esolve(f, Br, Bi, n, R, first=0, cnt=None, ld_u=None):
    """slod_lod_factor_solve_complex_ensemble out of place into two NaN-filled [nrow][ld_u]."""
    torch, dev = _torch()
    cnt = f.n_members - first if cnt is None else cnt
    ld_u = cnt * n if ld_u is None else ld_u
    ur, ui = _nan(Br.shape[0], ld_u), _nan(Br.shape[0], ld_u)
    f.solve_complex(Br.data_ptr(), _ptr(Bi), ur.data_ptr(), ui.data_ptr(), n_rhs=n, first_member=first, n_members=cnt,
                    rhs_members=R, ld_rhs=Br.shape[1], ld_u=ld_u)
    torch.cuda.synchronize()
    return ur, ui


def _single_solve(fk, Br, Bi, n, col0):
    """slod_lod_factor_solve_complex of a one-member factor on the columns col0 .. col0 + n - 1 of (Br, Bi)."""
    torch, dev = _torch()
    ur, ui = _nan(Br.shape[0], n), _nan(Br.shape[0], n)
    fk.solve_complex(_ptr(Br, col0), _ptr(Bi, col0), ur.data_ptr(), ui.data_ptr(), n_rhs=n, ld_rhs=Br.shape[1], ld_u=n)
    torch.cuda.synchronize()
    return ur, ui


# ---- 1. the factor against the yardstick, the solve against the bound, at every (damping, frequency, member)

@pytest.mark.parametrize("name,label", [("rowmajor", "mass"), ("rowmajor", "stiff"), ("rowmajor", "both"), ("base", "mass"),
                                        ("base", "stiff"), ("base", "both"), ("s2", "both")])
def test_ensemble_factor_and_solve_against_the_yardstick(so, name, label):
    c = he.harmonic_ensemble_case(so, name)
    b, K, rng = c.hbw, c.K, np.random.default_rng(701)
    dm, ds, freqs = c.sweep[label]
    F = len(freqs)
    assert F == 10 and K == 3
    omegas = np.array([w for w, _, _ in freqs])
    alpha, beta = hc.coefficients(omegas, dm, ds)
    f, A_t, M_t = _ensemble_factor(c, alpha, beta)
    assert (f.bad_pivot == -1).all() and f.n_members == F * K and len(f.bad_pivot) == F * K
    assert (f.info.n, f.info.half_bandwidth, f.info.block) == (c.nrow, b, 16)
    S = [[hc.system(c.A[m], c.M[m], w, dm, ds) for m in range(K)] for w in omegas]
    worst = dict(growth=0.0, norm=0.0, G=0.0, D=0.0, eta=0.0, solve=0.0, modal=0.0)
    for k, (w, refs, moves) in enumerate(freqs):
        if moves:
            print("%s %s: omega %d moved %d times to %.6e" % (name, label, k, moves, w))
        for m, ref in enumerate(refs):
            j = k * K + m
            ine, mi = f.inertia(j), f.member_info(j)
            assert (ine.n_negative, ine.n_positive) == (-1, -1)
            norm = float(np.abs(S[k][m]).astype(np.longdouble).sum(axis=1).max())
            d_norm = abs(ine.norm_matrix - norm) / norm
            assert d_norm <= (2 * b + 2) * hc.U, (name, label, k, m, d_norm)
            assert 0.5 * ref.G <= ine.norm_factor <= 2.0 * ref.G, (name, label, k, m, ine.norm_factor, ref.G)
            lo, hi = np.abs(ref.d).min(), np.abs(ref.d).max()
            d_D = max(abs(ine.min_abs_pivot - lo) / lo, abs(ine.max_abs_pivot - hi) / hi)
            assert d_D <= 1e-10, (name, label, k, m, d_D)
            assert (mi.min_pivot, mi.max_pivot) == (ine.min_abs_pivot, ine.max_abs_pivot)
            worst.update(growth=max(worst["growth"], ine.growth), norm=max(worst["norm"], d_norm), D=max(worst["D"], d_D),
                         G=max(worst["G"], abs(ine.norm_factor - ref.G) / ref.G))
    assert f.info.min_pivot == min(f.member_info(j).min_pivot for j in range(F * K))
    for n in (1, 3, 17):                                     # member m's own loads: the columns m n .. of the rhs
        hb, Br, Bi = _loads(rng, c.nrow, K * n)
        x = _z(*_esolve(f, Br, Bi, n, K))
        assert np.isfinite(x).all()
        for k, (w, refs, _) in enumerate(freqs):
            for m, ref in enumerate(refs):
                j = k * K + m
                xj, bm = x[:, j * n:(j + 1) * n], hb[:, m * n:(m + 1) * n]
                e = hc.zeta(S[k][m], ref.G, xj, bm)
                assert (e <= hc.ZBOUND * hc.bound(b)).all(), (name, label, k, m, n, e.max(), hc.ZBOUND * hc.bound(b))
                scale = np.abs(xj).max(axis=0)
                e_solve = (np.abs(xj - np.linalg.solve(S[k][m], bm)).max(axis=0) / scale).max()
                e_modal = (np.abs(xj - hc.modal_response(c.lam_h[m], c.X[m], bm, w, dm, ds)).max(axis=0) / scale).max()
                worst.update(eta=max(worst["eta"], e.max()), solve=max(worst["solve"], e_solve), modal=max(worst["modal"], e_modal))
                assert e_solve <= hc.FORWARD and e_modal <= hc.FORWARD, (name, label, k, m, n, e_solve, e_modal)
    print("%s %s: growth <= %.3e, norm_matrix off by %.2e, norm_factor by %.2e, |D| range by %.2e; backward error %.3e "
          "= %.4f of the bound %.3e; forward error %.3e (dense solve), %.3e (modal)"
          % (name, label, worst["growth"], worst["norm"], worst["G"], worst["D"], worst["eta"],
             worst["eta"] / (hc.ZBOUND * hc.bound(b)), hc.ZBOUND * hc.bound(b), worst["solve"], worst["modal"]))
    f.close()
    torch, dev = _torch()
    assert bool(torch.isnan(A_t[:, K:]).all()) and bool(torch.isnan(M_t[:, K:]).all())


# ---- 2. words: every factor member is the one-member factor of its (frequency, member); the rhs maps of the solve

@pytest.mark.parametrize("name", ["rowmajor", "base"])
def test_ensemble_factor_members_and_solve_words(so, name):
    import slod_amd
    torch, dev = _torch()
    c = he.harmonic_ensemble_case(so, name)
    g, K = c.g, c.K
    dm, ds, freqs = c.sweep["both"]
    omegas = np.array([w for w, _, _ in freqs])
    alpha, beta = hc.coefficients(omegas, dm, ds)
    F, n = len(omegas), 3
    J = F * K
    f, _, _ = _ensemble_factor(c, alpha, beta)
    hb, Br, Bi = _loads(np.random.default_rng(703), c.nrow, J * n)
    ref = _words(*_esolve(f, Br, Bi, n, J))                  # rhs_members = F K: every factor member its own columns
    assert np.isfinite(_z(*_esolve(f, Br, Bi, n, J))).all()
    assert np.array_equal(_words(*_esolve(f, Br, Bi, n, J)), ref)              # a repeated call
    for j in range(J):
        k, m = divmod(j, K)
        fk = g.lod_factor_zldl(c.sym[m].data_ptr(), c.mass[m].data_ptr(), c.cols.data_ptr(), alpha[k], beta[k])
        assert _info_words(fk, 0) == _info_words(f, j), (k, m)
        assert np.array_equal(_words(*_single_solve(fk, Br, Bi, n, j * n)), ref[:, :, j * n:(j + 1) * n]), (k, m)
        fk.close()

    def gathered(members, R):
        """What the members read with period R, from the distinct solve of the gathered columns (a column's bits depend on
        its member's factor and that rhs column only); members consecutive."""
        src = np.concatenate([(j % R) * n + np.arange(n) for j in members])
        idx = torch.from_numpy(src).to(dev)
        Gr, Gi = _nan(c.nrow, J * n), _nan(c.nrow, J * n)
        first = members[0]
        Gr[:, first * n:first * n + len(src)], Gi[:, first * n:first * n + len(src)] = Br[:, idx], Bi[:, idx]
        return _words(*_esolve(f, Gr, Gi, n, J, first=first, cnt=len(members)))

    everyone = list(range(J))
    for R in (1, K):
        assert np.array_equal(_words(*_esolve(f, Br, Bi, n, R)), gathered(everyone, R)), R
    # rhs_members = 1 is shared_rhs of the single-matrix call's interface
    ur, ui = _nan(c.nrow, J * n), _nan(c.nrow, J * n)
    f.solve_complex(Br.data_ptr(), Bi.data_ptr(), ur.data_ptr(), ui.data_ptr(), n_rhs=n, shared_rhs=True, ld_rhs=J * n)
    torch.cuda.synchronize()
    assert np.array_equal(_words(ur, ui), gathered(everyone, 1))
    # a member sub-range whose first member is no multiple of K, padded leading dimensions, NaN padding untouched
    sub = list(range(4, 11))
    Brw, Biw = _padded(Br, 5), _padded(Bi, 5)
    for R in (K, J):
        ur, ui = _esolve(f, Brw, Biw, n, R, first=4, cnt=7, ld_u=7 * n + 7)
        assert np.array_equal(_words(ur[:, :7 * n], ui[:, :7 * n]), gathered(sub, R)), R
        for t in (ur[:, 7 * n:], ui[:, 7 * n:], Brw[:, J * n:], Biw[:, J * n:]):
            assert bool(torch.isnan(t).all())
    # in place where every member reads the columns it writes
    for first, cnt, R in ((K, K, K), (0, J, J), (2 * K, 2, K)):
        Xr, Xi = _nan(c.nrow, cnt * n), _nan(c.nrow, cnt * n)
        src = torch.from_numpy(np.concatenate([(j % R) * n + np.arange(n) for j in range(first, first + cnt)])).to(dev)
        Xr[:], Xi[:] = Br[:, src], Bi[:, src]
        want = _words(*_esolve(f, Xr.clone(), Xi.clone(), n, R, first=first, cnt=cnt))
        f.solve_complex(Xr.data_ptr(), Xi.data_ptr(), Xr.data_ptr(), Xi.data_ptr(), n_rhs=n, first_member=first, n_members=cnt,
                        rhs_members=R, ld_rhs=cnt * n)
        torch.cuda.synchronize()
        assert np.array_equal(_words(Xr, Xi), want), (first, cnt, R)
    # and refused where two members read the same columns, or a member would read what another writes
    ur, ui = _nan(c.nrow, J * n), _nan(c.nrow, J * n)
    for kw in (dict(first_member=0, n_members=K + 1, rhs_members=K), dict(first_member=0, n_members=2, rhs_members=1),
               dict(first_member=4, n_members=2, rhs_members=K)):
        for rhs, u in (((ur, ui), (ur, ui)), ((ur, None), (ur, ui)), ((ur, ui), (Br, ui))):
            with pytest.raises(slod_amd.SlodError) as e:
                f.solve_complex(rhs[0].data_ptr(), _ptr(rhs[1]), u[0].data_ptr(), u[1].data_ptr(), n_rhs=n, ld_rhs=J * n, ld_u=J * n, **kw)
            assert e.value.code == -1 and "slod_lod_factor_solve_complex_ensemble:" in str(e.value) and "in place" in str(e.value)
    # the other refusals that read the factor
    for kw, word in ((dict(rhs_members=0), "rhs_members < 1"), (dict(rhs_members=-2), "rhs_members < 1"),
                     (dict(first_member=J - 1, n_members=2, rhs_members=1), "members outside the factor"),
                     (dict(first_member=-1, rhs_members=1), "members outside"), (dict(rhs_members=K, ld_u=J * n - 1), "leading dimension of u"),
                     (dict(rhs_members=K, ld_rhs=K * n - 1), "leading dimension of the rhs"),
                     (dict(rhs_members=J, ld_rhs=J * n - 1), "leading dimension of the rhs"), (dict(rhs_members=1, n_rhs=0), "n_rhs < 1")):
        args = dict(n_rhs=n)
        args.update(kw)
        with pytest.raises(slod_amd.SlodError) as e:
            f.solve_complex(Br.data_ptr(), Bi.data_ptr(), ur.data_ptr(), ui.data_ptr(), **args)
        assert e.value.code == -1 and "slod_lod_factor_solve_complex_ensemble:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    for real in (g.lod_factor(c.sym[0].data_ptr(), c.cols.data_ptr()), g.lod_factor_ldl(c.sym[0].data_ptr(), c.cols.data_ptr())):
        rc = g.lib.slod_lod_factor_solve_complex_ensemble(real.f, 0, 1, Br.data_ptr(), None, 1, 1, 1, ur.data_ptr(), ui.data_ptr(), 1, None)
        msg = g.lib.slod_last_error(g.h).decode()
        assert rc == -1 and msg.startswith("slod_lod_factor_solve_complex_ensemble: a real factor"), msg
        real.close()
    # a second factor has the same words
    f2, _, _ = _ensemble_factor(c, alpha, beta, pads=(0, 1))
    assert np.array_equal(_words(*_esolve(f2, Br, Bi, n, J)), ref)
    assert [_info_words(f, j) for j in range(J)] == [_info_words(f2, j) for j in range(J)]
    f2.close()
    f.close()


# ---- 3. the response call

def _response(c, A_t, M_t, K, w, dm, ds, Lr, Li, n, pad_u=2):
    """The call on NaN-padded u (ld_u = F K n + pad_u); the loads (Lr, Li) have their own padding."""
    torch, dev = _torch()
    F = len(w)
    ur, ui = _nan(c.nrow, F * K * n + pad_u), _nan(c.nrow, F * K * n + pad_u)
    res, growth, q = c.g.lod_harmonic_response_ensemble(
        A_t.data_ptr(), M_t.data_ptr(), c.cols.data_ptr(), K, w, Lr.data_ptr(), _ptr(Li), ur.data_ptr(), ui.data_ptr(), n_rhs=n,
        damp_mass=dm, damp_stiff=ds, ld_a_m=A_t.shape[1], ld_m_m=M_t.shape[1], ld_load=Lr.shape[1], ld_u=F * K * n + pad_u)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ur[:, F * K * n:]).all()) and bool(torch.isnan(ui[:, F * K * n:]).all())
    assert res.shape == (F, K, n) and growth.shape == (F, K) and q.shape == (F, K, n, 4)
    return ur[:, :F * K * n], ui[:, :F * K * n], res, growth, q


def _single_response(c, sym, mass, w, dm, ds, Lr, Li, col0, n):
    """slod_lod_harmonic_response at the single frequency w on one member's matrices and load columns."""
    torch, dev = _torch()
    ur, ui = _nan(c.nrow, n), _nan(c.nrow, n)
    res, growth = c.g.lod_harmonic_response(sym.data_ptr(), mass.data_ptr(), c.cols.data_ptr(), [w], _ptr(Lr, col0), _ptr(Li, col0),
                                            ur.data_ptr(), ui.data_ptr(), n_rhs=n, damp_mass=dm, damp_stiff=ds, ld_load=Lr.shape[1])
    torch.cuda.synchronize()
    return _words(ur, ui), res[0], growth[0]


def _check_against_the_single_call(c, singles, K, w, dm, ds, Lr, Li, n, got):
    ur, ui, res, growth, q = got
    words = _words(ur, ui)
    for k in range(len(w)):
        for m in range(K):
            one, r1, g1 = _single_response(c, singles[m][0], singles[m][1], w[k], dm, ds, Lr, Li, m * n, n)
            at = he.column(k, m, 0, K, n)
            assert np.array_equal(one, words[:, :, at:at + n]), (k, m, n)
            assert r1.tobytes() == res[k, m].tobytes() and np.float64(g1).tobytes() == growth[k, m].tobytes(), (k, m, n)


def _check_numbers(c, dense, K, w, dm, ds, load, n, got, label):
    """rel_residual against the extended-precision residual, quantities against numpy longdouble, the power identity."""
    ur, ui, res, growth, q = got
    x = he.deinterleave(_z(ur, ui), len(w), K, n)
    worst = dict(res=0.0, q=0.0, power=0.0)
    for k in range(len(w)):
        for m in range(K):
            A, M = dense(m)
            S = hc.system(A, M, w[k], dm, ds)
            xk, bm = x[:, k, m, :], load[:, m * n:(m + 1) * n]
            r = bm.astype(np.clongdouble) - S.astype(np.clongdouble) @ xk.astype(np.clongdouble)
            true = np.array(np.sqrt((np.abs(r) ** 2).sum(axis=0)) / np.linalg.norm(bm, axis=0), dtype=np.float64)
            room = 64 * hc.U * (np.abs(S).sum(axis=1).max() * np.linalg.norm(xk, axis=0) / np.linalg.norm(bm, axis=0) + 1.0)
            assert (np.abs(res[k, m] - true) <= np.maximum(1e-6 * true, room)).all(), (label, n, k, m, res[k, m], true)
            model = he.quantities_model(A, M, xk, bm)
            bars = he.quantities_bars(A, M, xk, bm, c.nrow, c.cap * c.s)
            off = np.array(np.abs(q[k, m].astype(np.longdouble) - model), dtype=np.float64)
            assert (off <= bars).all(), (label, n, k, m, off, bars)
            ub = np.abs(q[k, m, :, 2] + 1j * q[k, m, :, 3])
            power = w[k] * (dm * q[k, m, :, 0] + ds * q[k, m, :, 1])
            assert (np.abs(power - q[k, m, :, 3]) <= 1e-8 * ub).all(), (label, n, k, m, power, q[k, m, :, 3])
            worst.update(res=max(worst["res"], res[k, m].max()), q=max(worst["q"], (off / bars).max()),
                         power=max(worst["power"], (np.abs(power - q[k, m, :, 3]) / ub).max()))
    print("%s n_rhs %d: residual <= %.3e, growth <= %.3e, quantities at %.3f of their bars, power identity off by %.3e"
          % (label, n, worst["res"], growth.max(), worst["q"], worst["power"]))


_sweep23 = {}


def _base23(so):
    """base with the ten frequencies of the rule and 13 evenly spaced ones at the damping `both`, jointly qualified; the
    loads: column m n + 0 the load of member m's first mode (real), the others random complex."""
    c = he.harmonic_ensemble_case(so, "base")
    if not _sweep23:
        dm, ds, freqs = he.ensemble_sweep(c.lam_h, c.A, c.M, c.perm, extra=13)["both"]
        rng = np.random.default_rng(705)
        loads = {}
        for n in (1, 3):
            hb = rng.uniform(-1.0, 1.0, (c.nrow, c.K * n)) + 1j * rng.uniform(-1.0, 1.0, (c.nrow, c.K * n))
            for m in range(c.K):
                hb[:, m * n] = c.M[m] @ c.X[m][:, 0]
            if n == 1:
                hb = hb.real + 0j
            loads[n] = hb
        _sweep23.update(dm=dm, ds=ds, freqs=freqs, loads=loads)
    return c, _sweep23


def test_response_ensemble_across_a_chunk_boundary_inside_a_frequency(so):
    torch, dev = _torch()
    c, sw = _base23(so)
    K, dm, ds, freqs = c.K, sw["dm"], sw["ds"], sw["freqs"]
    w = np.array([x for x, _, _ in freqs])
    F = len(w)
    assert F == 23 and he.chunks(F, K) == [(0, 64), (64, 69)] and divmod(64, K) == (21, 1)
    moved = [(k, m) for k, (_, _, m) in enumerate(freqs) if m]
    print("base: %d of 23 frequencies moved %r; worst yardstick growth %.3e"
          % (len(moved), moved, max(r.G / r.norm for _, refs, _ in freqs for r in refs)))
    A_t, M_t = he.stack(c, c.sym, K, pad=2), he.stack(c, c.mass, K, pad=5)
    singles = [(c.sym[m], c.mass[m]) for m in range(K)]
    for n in (1, 3):
        hb = sw["loads"][n]
        Lr, Li = _padded(_dev(hb.real), 1), (_padded(_dev(hb.imag), 1) if n > 1 else None)
        got = _response(c, A_t, M_t, K, w, dm, ds, Lr, Li, n)
        _check_against_the_single_call(c, singles, K, w, dm, ds, Lr, Li, n, got)
        _check_numbers(c, lambda m: (c.A[m], c.M[m]), K, w, dm, ds, hb, n, got, "base K = 3, F = 23")
        ref = _words(got[0], got[1])
        # a repeated call
        again = _response(c, A_t, M_t, K, w, dm, ds, Lr, Li, n)
        assert np.array_equal(_words(again[0], again[1]), ref)
        for a, b in zip(got[2:], again[2:]):
            assert a.tobytes() == b.tobytes()
        # F = 1: a frequency alone is its block of the sweep
        for k in (0, 21):
            one = _response(c, A_t, M_t, K, w[k:k + 1], dm, ds, Lr, Li, n)
            assert np.array_equal(_words(one[0], one[1]), ref[:, :, k * K * n:(k + 1) * K * n]), (n, k)
            assert one[2][0].tobytes() == got[2][k].tobytes() and one[3][0].tobytes() == got[3][k].tobytes()
            assert one[4][0].tobytes() == got[4][k].tobytes()
        # permuted members: the columns, the residuals, the growths and the quantities move with them
        order = [2, 0, 1]
        Ap = he.stack(c, [c.sym[m] for m in order], K, pad=0)
        Mp = he.stack(c, [c.mass[m] for m in order], K, pad=1)
        cols = np.concatenate([m * n + np.arange(n) for m in order])
        hp = hb[:, cols]
        pr, pi, pres, pgrowth, pq = _response(c, Ap, Mp, K, w, dm, ds, _dev(hp.real), _dev(hp.imag) if n > 1 else None, n, pad_u=0)
        full = np.concatenate([he.column(k, m, 0, K, n) + np.arange(n) for k in range(F) for m in order])
        assert np.array_equal(_words(pr, pi), ref[:, :, full]), n
        assert pres.tobytes() == got[2][:, order].tobytes() and pgrowth.tobytes() == got[3][:, order].tobytes()
        assert pq.tobytes() == got[4][:, order].tobytes()
        # each member's amplitude curve peaks at the sample nearest its own first resonance
        amp = np.sqrt(got[4][:, :, 0, 0])
        for m in range(K):
            nearest = int(np.argmin(np.abs(w - np.sqrt(c.lam_h[m][0]))))
            assert int(np.argmax(amp[:, m])) == nearest, (n, m, int(np.argmax(amp[:, m])), nearest)
    # a zero load column: u = 0, residual 0 and four exact zeros
    Z = torch.zeros((c.nrow, K * 2), dtype=torch.float64, device=dev)
    Z[:, 1::2] = _dev(sw["loads"][1].real)
    ur, ui, res, growth, q = _response(c, A_t, M_t, K, w[:2], dm, ds, Z, None, 2)
    assert bool((ur[:, 0::2] == 0.0).all()) and bool((ui[:, 0::2] == 0.0).all())
    assert (res[:, :, 0] == 0.0).all() and (res[:, :, 1] > 0.0).all() and (q[:, :, 0, :] == 0.0).all() and (q[:, :, 1, 0] > 0.0).all()


def test_response_ensemble_of_65_members_and_two_frequencies(so):
    torch, dev = _torch()
    c = he.harmonic_ensemble_case(so, "base")
    K, F = 65, 2
    assert he.chunks(F, K) == [(0, 64), (64, 128), (128, 130)]
    scale = [1.0 if k < c.K else 1.0 + k / 64.0 for k in range(K)]           # the factors of stack()

    def dense(m):
        return c.A[m % c.K] * scale[m], c.M[m % c.K] * scale[m]

    lam = c.lam_h[0]
    _, dm, ds = hc.dampings(lam)[2]
    rule = hc.rule_frequencies(lam)
    As, Ms = zip(*[dense(m) for m in range(K)])
    freqs = [he.qualify_joint(As, Ms, x, dm, ds, c.perm) for x in (rule[5], rule[6])]
    print("base K = 65: moves %r, worst yardstick growth %.3e" % ([mv for _, _, mv in freqs], max(r.G / r.norm for _, refs, _ in freqs for r in refs)))
    w = np.array([x for x, _, _ in freqs])
    A_t, M_t = he.stack(c, c.sym, K, pad=2), he.stack(c, c.mass, K, pad=5)
    singles = [(A_t[:, m].contiguous(), M_t[:, m].contiguous()) for m in range(K)]
    rng = np.random.default_rng(707)
    for n in (1, 3):
        hb = rng.uniform(-1.0, 1.0, (c.nrow, K * n)) + 1j * rng.uniform(-1.0, 1.0, (c.nrow, K * n))
        if n == 1:
            hb = hb.real + 0j
        Lr, Li = _padded(_dev(hb.real), 1), (_padded(_dev(hb.imag), 1) if n > 1 else None)
        got = _response(c, A_t, M_t, K, w, dm, ds, Lr, Li, n)
        _check_against_the_single_call(c, singles, K, w, dm, ds, Lr, Li, n, got)
        _check_numbers(c, dense, K, w, dm, ds, hb, n, got, "base K = 65, F = 2")
    assert bool(torch.isnan(A_t[:, K:]).all()) and bool(torch.isnan(M_t[:, K:]).all())


# ---- 4. failure: a status word, not a device fault

def test_response_ensemble_reports_the_failed_frequency_and_member(so):
    import slod_amd
    import lod_ldl_cases as lc
    torch, dev = _torch()
    c = he.harmonic_ensemble_case(so, "rowmajor")
    g, K = c.g, c.K
    dm, ds, freqs = c.sweep["both"]
    w = np.array([freqs[k][0] for k in (5, 6, 7)])
    F = len(w)
    alpha, beta = hc.coefficients(w, dm, ds)
    L = _dev(np.ones((c.nrow, K)))
    r = c.nrow // 2
    holed = [t.clone() for t in c.sym]
    holed[2][lc.diagonal_word(c, r)] = NAN                 # the diagonal entry of factor index r of member 2
    zeroed_a, zeroed_m = [t.clone() for t in c.sym], [t.clone() for t in c.mass]
    zeroed_a[1] *= 0.0
    zeroed_m[1] *= 0.0
    for what, sym, mass, member, pivot, value in (("zero member", zeroed_a, zeroed_m, 1, 0, r"\(0, 0\)"),
                                                  ("NaN", holed, c.mass, 2, r, r"\((-?nan), (.*)\)")):
        A_t, M_t = he.stack(c, sym, K, pad=1), he.stack(c, mass, K, pad=0)
        want = [pivot if j % K == member else -1 for j in range(F * K)]
        out, bad = C.c_void_p(1), np.full(F * K, 7, dtype=np.int32)
        ap, bp = np.ascontiguousarray(alpha).view(np.float64), np.ascontiguousarray(beta).view(np.float64)
        rc = g.lib.slod_lod_factor_create_zldl_ensemble(g.h, A_t.data_ptr(), K + 1, M_t.data_ptr(), K, K, c.cols.data_ptr(),
                                                        ap.ctypes.data_as(C.POINTER(C.c_double)), bp.ctypes.data_as(C.POINTER(C.c_double)),
                                                        F, bad.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(out))
        msg = g.lib.slod_last_error(g.h).decode()
        print("%s: %d, %s" % (what, rc, msg))
        assert rc == -5 and out.value is None and list(bad) == want, (what, rc, list(bad))
        assert re.fullmatch(r"slod_lod_factor_create_zldl_ensemble: coefficient 0, member %d: pivot %d of %d is zero or not finite %s"
                            % (member, pivot, c.nrow, value), msg), msg
        with pytest.raises(slod_amd.SlodError) as e:
            g.lod_factor_zldl_ensemble(A_t.data_ptr(), M_t.data_ptr(), c.cols.data_ptr(), K, alpha, beta, ld_a_m=K + 1)
        assert e.value.code == -5 and list(e.value.bad_pivot) == want
        ur, ui = _nan(c.nrow, F * K), _nan(c.nrow, F * K)
        with pytest.raises(slod_amd.SlodError) as e:
            g.lod_harmonic_response_ensemble(A_t.data_ptr(), M_t.data_ptr(), c.cols.data_ptr(), K, w, L.data_ptr(), None, ur.data_ptr(),
                                             ui.data_ptr(), damp_mass=dm, damp_stiff=ds, ld_a_m=K + 1)
        assert e.value.code == -5, str(e.value)
        assert re.search(r"slod_lod_harmonic_response_ensemble: frequency 0, member %d: pivot %d of %d is zero or not finite %s$"
                         % (member, pivot, c.nrow, value), str(e.value)), str(e.value)
        # the same call without that member succeeds with finite output
        keep = [m for m in range(K) if m != member]
        A2, M2 = he.stack(c, [sym[m] for m in keep], 2, pad=0), he.stack(c, [mass[m] for m in keep], 2, pad=0)
        ur, ui = _nan(c.nrow, F * 2), _nan(c.nrow, F * 2)
        res, growth, q = g.lod_harmonic_response_ensemble(A2.data_ptr(), M2.data_ptr(), c.cols.data_ptr(), 2, w, L.data_ptr(), None,
                                                          ur.data_ptr(), ui.data_ptr(), damp_mass=dm, damp_stiff=ds, ld_load=K)
        torch.cuda.synchronize()
        assert np.isfinite(res).all() and np.isfinite(growth).all() and np.isfinite(q).all()
        assert bool(torch.isfinite(ur).all()) and bool(torch.isfinite(ui).all())


def test_real_consumers_refuse_the_ensemble_complex_factor(so):
    import slod_amd
    torch, dev = _torch()
    c = he.harmonic_ensemble_case(so, "rowmajor")
    g = c.g
    f, _, _ = _ensemble_factor(c, [1.0 + 0.1j], [-1.0 + 0.2j])
    assert f.n_members == c.K
    text = "a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex"
    U0, V0, A0 = (_dev(np.ones((c.nrow, c.K))) for _ in range(3))
    X = _nan(c.nrow, 8)
    sym, mass, cols = c.sym[0].data_ptr(), c.mass[0].data_ptr(), c.cols.data_ptr()
    calls = {
        "slod_lod_factor_solve": lambda: g._check(g.lib.slod_lod_factor_solve(f.f, U0.data_ptr(), c.K, 1, V0.data_ptr(), c.K, None)),
        "slod_lod_factor_solve_ensemble": lambda: slod_amd.EnsembleFactor.solve(f, U0.data_ptr(), V0.data_ptr()),
        "slod_lod_theta_steps_direct": lambda: g.lod_theta_steps_direct(f, sym, cols, 0.01, 0.5, 1, U0.data_ptr(), ld_u=c.K),
        "slod_lod_eigs_direct": lambda: g.lod_eigs_direct(f, sym, mass, cols, 2, X.data_ptr(), n_block=8),
        "slod_lod_eigs_shift_direct": lambda: g.lod_eigs_shift_direct(f, 1.0, sym, mass, cols, 2, X.data_ptr(), n_block=8),
        "slod_lod_solve_multi_precond": lambda: g.lod_solve_multi_precond(f, sym, cols, U0.data_ptr(), c.K, 1, V0.data_ptr(), c.K),
    }
    for who, call in calls.items():
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith(who + ": " + text), (who, str(e.value))
    assert bool((U0 == 1.0).all()) and bool((V0 == 1.0).all())
    f.close()


# ---- 5. end to end

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


def test_harmonic_pipeline_equals_three_single_pipelines(so):
    torch, dev = _torch()
    c = he.harmonic_ensemble_case(so, "rowmajor")
    g, K = c.g, c.K
    dm, ds, freqs = c.sweep["both"]
    w = np.array([freqs[k][0] for k in (5, 0, 6)])
    F = len(w)
    V, M, A = (_nan(c.nval, K) for _ in range(3))
    cols, mcols = torch.zeros_like(c.cols), torch.zeros_like(c.cols)
    load = torch.zeros(c.field, dtype=torch.float64, device=dev)
    g.fem_rhs(None, load.data_ptr())
    R = _nan(c.nrow, K)
    ur, ui = _nan(c.nrow, F * K), _nan(c.nrow, F * K)
    g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix_ensemble(c.b.data_ptr(), c.stride, K, M.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, A.data_ptr())
    g.lod_rhs_ensemble(c.b.data_ptr(), c.stride, K, load.data_ptr(), R.data_ptr())
    res, growth, q = g.lod_harmonic_response_ensemble(A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, w, R.data_ptr(), None,
                                                      ur.data_ptr(), ui.data_ptr(), damp_mass=dm, damp_stiff=ds)
    fields, moments = {}, {}
    for k in range(F):                                      # a frequency's block is an ensemble multi-vector at offset k K
        for part, u in (("re", ur), ("im", ui)):
            fine, mean, var = _nan(K, c.field), _nan(1, c.field), _nan(1, c.field)
            g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, K, _ptr(u, k * K), fine.data_ptr(), ld_u=F * K)
            g.ensemble_moments(fine.data_ptr(), K, c.field, mean.data_ptr(), var.data_ptr())
            torch.cuda.synchronize()
            fields[k, part], moments[k, part] = fine, (mean, var)
    assert torch.equal(cols, c.cols) and torch.equal(mcols, c.cols)
    single = {(k, part): [] for k in range(F) for part in ("re", "im")}
    for m in range(K):
        rhs = _nan(c.nrow, 1)
        g.lod_rhs(np.arange(c.NP), c.slab[m][0].data_ptr(), c.stride, load.data_ptr(), rhs.data_ptr())
        sr, si = _nan(c.nrow, F), _nan(c.nrow, F)
        res1, growth1 = g.lod_harmonic_response(c.sym[m].data_ptr(), c.mass[m].data_ptr(), c.cols.data_ptr(), w, rhs.data_ptr(), None,
                                                sr.data_ptr(), si.data_ptr(), damp_mass=dm, damp_stiff=ds)
        torch.cuda.synchronize()
        assert res1[:, 0].tobytes() == np.ascontiguousarray(res[:, m, 0]).tobytes()
        assert growth1.tobytes() == np.ascontiguousarray(growth[:, m]).tobytes()
        for k in range(F):
            assert np.array_equal(_bits(sr[:, k]), _bits(ur[:, k * K + m])) and np.array_equal(_bits(si[:, k]), _bits(ui[:, k * K + m]))
            for part, u in (("re", sr), ("im", si)):
                out = _nan(1, c.field)
                g.lod_reconstruct(c.slab[m][0].data_ptr(), c.stride, u[:, k].contiguous().data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                single[k, part].append(out[0].cpu().numpy())
    for key, rows in single.items():
        rows = np.stack(rows)
        assert np.isfinite(rows).all() and np.abs(rows).max() > 0.0
        assert np.array_equal(_bits(fields[key]), rows.view(np.uint64)), key
        mean, var = _moments_numpy(rows)
        assert np.array_equal(_bits(moments[key][0][0]), mean.view(np.uint64)), key
        assert np.array_equal(_bits(moments[key][1][0]), var.view(np.uint64)), key


# ---- 6. the mirror and the driver

def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", *args], capture_output=True, text=True, timeout=300)
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


LINE = r"omega = (\S+), growth = (\S+), relative residual = (\S+), amplitude = (\S+), power = (\S+)$"


def test_driver_ensemble_harmonic_matches_python_path_and_member_runs(so):
    """bin/main_Diffusion 3 4 1 1 --ensemble 3 --harmonic 5 W0 W1 --damping DM DS (W and the damping from member 0's
    lambda_1, as test_gpu_lod_harmonic.py chooses them) prints per (frequency, member) the growth, the residual, the
    amplitude and the dissipated power of the Python path to the digits printed; member M's lines are those of the
    --member M --harmonic run; then the amplitude's mean and deviation per frequency and the four field norms."""
    import scipy.linalg as sl
    import slod_amd
    from lod_cases import _rows_to_dense
    torch, dev = _torch()
    K, F = 3, 5
    kw = dict(nref=3, n_sub=4, oversampling=1, spacedim=1)
    g = slod_amd.Slod(n_problems=K, **kw)
    for k, field in enumerate(_driver_fields(so, g.NE, K)):
        g.set_coefficient(0, field, problem=k)
    NP, cap = g.num_patches, g.lod_row_capacity()
    plan = g.plan(np.arange(K * NP, dtype=np.uint32))
    b = torch.zeros(K * NP * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    nval, nrow = NP * cap, NP
    V, M, A = (_nan(nval, K) for _ in range(3))
    cols, mcols = (torch.zeros(nval, dtype=torch.int32, device=dev) for _ in range(2))
    load = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, load.data_ptr())
    R = _nan(nrow, K)
    g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), plan.stride, K, V.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix_ensemble(b.data_ptr(), plan.stride, K, M.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, A.data_ptr())
    g.lod_rhs_ensemble(b.data_ptr(), plan.stride, K, load.data_ptr(), R.data_ptr())
    torch.cuda.synchronize()
    hcols = cols.cpu().numpy().view(np.uint32)
    lam = sl.eigh(_rows_to_dense(g, A[:, 0].contiguous().cpu().numpy(), hcols, 1),
                  _rows_to_dense(g, M[:, 0].contiguous().cpu().numpy(), hcols, 1), eigvals_only=True)
    w1 = float(np.sqrt(lam[0]))
    w0, wK, dm, ds = 0.5 * w1, 2.0 * w1, 0.02 * w1, 1e-3 / w1
    sweep = ["--harmonic", str(F), repr(w0), repr(wK), "--damping", repr(dm), repr(ds)]
    out = _driver("--ensemble", str(K), *sweep)
    lines = re.findall(r"^harmonic (\d+) member (\d+): " + LINE, out, re.M)
    assert [(int(x[0]), int(x[1])) for x in lines] == [(k, m) for k in range(1, F + 1) for m in range(K)], out
    # the Python path, the driver's frequencies
    omegas = np.array([w0 + k * ((wK - w0) / (F - 1)) for k in range(F)])
    ur, ui = _nan(nrow, F * K), _nan(nrow, F * K)
    res, growth, quant = g.lod_harmonic_response_ensemble(A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, omegas, R.data_ptr(), None,
                                                         ur.data_ptr(), ui.data_ptr(), damp_mass=dm, damp_stiff=ds)
    amp, power = np.zeros((F, K)), np.zeros((F, K))
    for k in range(F):                                      # as the mirror: slod_lod_inner_ensemble on the frequency's block
        uMu = sum(g.lod_inner_ensemble(M.data_ptr(), cols.data_ptr(), _ptr(t, k * K), _ptr(t, k * K), K, ld_x=F * K, ld_y=F * K)
                  for t in (ur, ui))
        uAu = sum(g.lod_inner_ensemble(A.data_ptr(), cols.data_ptr(), _ptr(t, k * K), _ptr(t, k * K), K, ld_x=F * K, ld_y=F * K)
                  for t in (ur, ui))
        amp[k], power[k] = np.sqrt(uMu), 0.5 * omegas[k] * (dm * uMu + ds * uAu)
    assert np.abs(amp - np.sqrt(quant[:, :, 0, 0])).max() <= 1e-12 * amp.max()          # the call's own u^H M u
    for x in lines:
        k, m = int(x[0]) - 1, int(x[1])
        want = ("%.12e" % omegas[k], "%.6e" % growth[k, m], "%.6e" % res[k, m, 0], "%.12e" % amp[k, m], "%.12e" % power[k, m])
        assert tuple(x[2:]) == want, (k, m, x, want)
    # member M's lines are those of the single run on member M's coefficient
    for m in range(K):
        single = re.findall(r"^harmonic (\d+): " + LINE, _driver("--member", str(m), *sweep), re.M)
        assert [int(x[0]) for x in single] == list(range(1, F + 1))
        assert [x[1:] for x in single] == [x[2:] for x in lines if int(x[1]) == m], m
    # mean and deviation of the amplitude per frequency, then the field norms of the loudest frequency
    stats = re.findall(r"^harmonic (\d+) amplitude over the ensemble of 3: mean = (\S+), standard deviation = (\S+)$", out, re.M)
    assert [int(x[0]) for x in stats] == list(range(1, F + 1)), out
    for k, x in enumerate(stats):
        assert abs(float(x[1]) - amp[k].mean()) <= 1e-11 * amp[k].mean() and abs(float(x[2]) - amp[k].std(ddof=1)) <= 1e-9 * amp[k].mean()
    peak = int(np.argmax(amp.mean(axis=1)))
    m = re.search(r"^SLOD harmonic ensemble of 3 at omega = (\S+): L2 norm of the mean = (\S+) \(real\), (\S+) \(imaginary\), of the "
                  r"standard deviation = (\S+) \(real\), (\S+) \(imaginary\)$", out, re.M)
    assert m and m.group(1) == "%.12e" % omegas[peak], out
    assert all(float(v) > 0.0 and np.isfinite(float(v)) for v in m.groups()[1:])
    g.close()
