"""GPU tests of the frequency response on the LOD space: the complex symmetric banded LDL^T
(slod_lod_factor_create_zldl, slod_lod_factor_solve_complex) and the sweep call (slod_lod_harmonic_response), against the
unpivoted complex LDL^T in numpy and the modal response of lod_harmonic_cases.py (checked on the CPU by
test_lod_harmonic_reference.py), numpy.linalg.solve, the real LDL^T factor, and itself as 64-bit words.

Cases: the four of test_gpu_lod_ldl.py with their real sym(A) and M (dense 16 rows, rowmajor 25, s2 128, morton16 256),
each at the eight frequencies of the sweep rule and the three dampings of lod_harmonic_cases.py; the growth cap is
asserted on the yardstick before the library is called.  The bars are those of lod_harmonic_cases.py; the figures the
tests print are recorded in DESIGN section 6.
"""
import ctypes as C
import re

import numpy as np
import pytest

import lod_harmonic_cases as hc
import lod_ldl_cases as lc
from lod_cases import NAN, _bits, _torch

pytestmark = pytest.mark.gpu


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _nan(rows, ld):
    torch, dev = _torch()
    return torch.full((rows, ld), NAN, dtype=torch.float64, device=dev)


def _ptr(t, first=0):
    return None if t is None else t.data_ptr() + 8 * first


def _factor(c, alpha, beta):
    return c.g.lod_factor_zldl(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), alpha, beta)


def _solve(f, Br, Bi, n, K=None, first=0, shared=False, ld_u=None, col0=0):
    """Out of place into two NaN-filled [nrow][ld_u]; the rhs from column col0 of (Br, Bi), Bi may be None."""
    torch, dev = _torch()
    K = f.n_members - first if K is None else K
    ld_u = K * n if ld_u is None else ld_u
    ur, ui = _nan(Br.shape[0], ld_u), _nan(Br.shape[0], ld_u)
    f.solve_complex(_ptr(Br, col0), _ptr(Bi, col0), ur.data_ptr(), ui.data_ptr(), n_rhs=n, first_member=first, n_members=K,
                    shared_rhs=shared, ld_rhs=Br.shape[1], ld_u=ld_u)
    torch.cuda.synchronize()
    return ur, ui


def _z(ur, ui):
    return ur.cpu().numpy() + 1j * ui.cpu().numpy()


def _words(ur, ui):
    return np.stack([_bits(ur), _bits(ui)])


def _info_words(f, k):
    i, m = f.inertia(k), f.member_info(k)
    assert (i.n_negative, i.n_positive) == (-1, -1)
    return np.array([i.min_abs_pivot, i.max_abs_pivot, i.norm_matrix, i.norm_factor, m.min_pivot, m.max_pivot]).tobytes()


def _loads(rng, rows, n, complex_load):
    hr = rng.uniform(-1.0, 1.0, (rows, n))
    hi = rng.uniform(-1.0, 1.0, (rows, n)) if complex_load else np.zeros((rows, n))
    return hr + 1j * hi, _dev(hr), _dev(hi) if complex_load else None


# ---- the factor against the yardstick, the solve against the bound, at every (damping, omega) of the rule

@pytest.mark.parametrize("name", lc.CASES)
def test_zldl_factor_and_solve_against_the_yardstick(so, name):
    c = hc.harmonic_case(so, name)
    b, rng = c.hbw, np.random.default_rng(501)
    for label, (dm, ds, freqs) in c.sweep.items():
        omegas = np.array([w for w, _, _ in freqs])
        alpha, beta = hc.coefficients(omegas, dm, ds)
        f = _factor(c, alpha, beta)
        assert (f.bad_pivot == -1).all() and f.n_members == 8
        assert (f.info.n, f.info.half_bandwidth, f.info.block) == (c.nrow, b, 16)
        S = [hc.system(c.A, c.M, w, dm, ds) for w in omegas]
        worst = dict(growth=0.0, norm=0.0, G=0.0, D=0.0, eta=0.0, solve=0.0, modal=0.0)
        for k, (w, ref, moves) in enumerate(freqs):
            ine, mi = f.inertia(k), f.member_info(k)
            assert (ine.n_negative, ine.n_positive) == (-1, -1)
            norm = float(np.abs(S[k]).astype(np.longdouble).sum(axis=1).max())
            d_norm = abs(ine.norm_matrix - norm) / norm
            assert d_norm <= (2 * b + 2) * hc.U, (name, label, k, d_norm)
            assert 0.5 * ref.G <= ine.norm_factor <= 2.0 * ref.G, (name, label, k, ine.norm_factor, ref.G)
            lo, hi = np.abs(ref.d).min(), np.abs(ref.d).max()
            d_D = max(abs(ine.min_abs_pivot - lo) / lo, abs(ine.max_abs_pivot - hi) / hi)
            assert d_D <= 1e-10, (name, label, k, d_D)
            assert (mi.min_pivot, mi.max_pivot) == (ine.min_abs_pivot, ine.max_abs_pivot)
            worst.update(growth=max(worst["growth"], ine.growth), norm=max(worst["norm"], d_norm), D=max(worst["D"], d_D),
                         G=max(worst["G"], abs(ine.norm_factor - ref.G) / ref.G))
            if moves:
                print("%s %s: omega %d moved %d times to %.6e" % (name, label, k, moves, w))
        assert f.info.min_pivot == min(f.member_info(k).min_pivot for k in range(8))
        for n in (1, 3, 16, 17):
            for complex_load in (False, True):
                hb, Br, Bi = _loads(rng, c.nrow, n, complex_load)
                x = _z(*_solve(f, Br, Bi, n, shared=True))
                assert np.isfinite(x).all()
                for k, (w, ref, _) in enumerate(freqs):
                    xk = x[:, k * n:(k + 1) * n]
                    e = hc.zeta(S[k], ref.G, xk, hb)
                    assert (e <= hc.ZBOUND * hc.bound(b)).all(), (name, label, k, n, e.max(), hc.ZBOUND * hc.bound(b))
                    scale = np.abs(xk).max(axis=0)
                    e_solve = (np.abs(xk - np.linalg.solve(S[k], hb)).max(axis=0) / scale).max()
                    e_modal = (np.abs(xk - hc.modal_response(c.lam_h, c.X, hb, w, dm, ds)).max(axis=0) / scale).max()
                    worst.update(eta=max(worst["eta"], e.max()), solve=max(worst["solve"], e_solve),
                                 modal=max(worst["modal"], e_modal))
                    assert e_solve <= hc.FORWARD and e_modal <= hc.FORWARD, (name, label, k, n, e_solve, e_modal)
        print("%s %s: growth <= %.3e, norm_matrix off by %.2e, norm_factor by %.2e, |D| range by %.2e; backward error %.3e "
              "= %.4f of the bound %.3e; forward error %.3e (dense solve), %.3e (modal)"
              % (name, label, worst["growth"], worst["norm"], worst["G"], worst["D"], worst["eta"],
                 worst["eta"] / (hc.ZBOUND * hc.bound(b)), hc.ZBOUND * hc.bound(b), worst["solve"], worst["modal"]))
        f.close()


# ---- words

@pytest.mark.parametrize("name", ["rowmajor", "morton16"])
def test_zldl_solve_words(so, name):
    torch, dev = _torch()
    c = hc.harmonic_case(so, name)
    dm, ds, freqs = c.sweep["both"]
    omegas = np.array([freqs[k][0] for k in (0, 6, 3)])
    alpha, beta = hc.coefficients(omegas, dm, ds)
    K, n = 3, 17
    f = _factor(c, alpha, beta)
    rng = np.random.default_rng(503)
    hb, Br, Bi = _loads(rng, c.nrow, K * n, True)
    ref = _words(*_solve(f, Br, Bi, n))
    assert np.isfinite(_z(*_solve(f, Br, Bi, n))).all()
    # a repeated solve
    assert np.array_equal(_words(*_solve(f, Br, Bi, n)), ref)
    # a column as its own n_rhs = 1 run of its member
    for k, j in ((0, 0), (1, 2), (1, 15), (2, 16), (0, 16)):
        one = _words(*_solve(f, Br, Bi, 1, K=1, first=k, col0=k * n + j))
        assert np.array_equal(one[:, :, 0], ref[:, :, k * n + j]), (k, j)
    # permuted columns inside every member
    perm = rng.permutation(n)
    full = np.concatenate([k * n + perm for k in range(K)])
    idx = torch.from_numpy(full).to(dev)
    got = _words(*_solve(f, Br[:, idx].contiguous(), Bi[:, idx].contiguous(), n))
    assert np.array_equal(got, ref[:, :, full])
    # padded leading dimensions, NaN padding left untouched
    Brw, Biw = _nan(c.nrow, K * n + 5), _nan(c.nrow, K * n + 5)
    Brw[:, :K * n], Biw[:, :K * n] = Br, Bi
    ur, ui = _solve(f, Brw, Biw, n, ld_u=K * n + 7)
    assert np.array_equal(_words(ur[:, :K * n], ui[:, :K * n]), ref)
    for t in (ur[:, K * n:], ui[:, K * n:], Brw[:, K * n:], Biw[:, K * n:]):
        assert bool(torch.isnan(t).all())
    # a member sub-range
    got = _words(*_solve(f, Br, Bi, n, K=2, first=1, col0=n))
    assert np.array_equal(got, ref[:, :, n:])
    # a shared rhs equals the load copied per member; a real shared rhs equals a zero imaginary plane
    Sr, Si = Br[:, :n].contiguous(), Bi[:, :n].contiguous()
    shared = _words(*_solve(f, Sr, Si, n, shared=True))
    assert np.array_equal(shared, _words(*_solve(f, Sr.repeat(1, K), Si.repeat(1, K), n)))
    assert np.array_equal(_words(*_solve(f, Sr, None, n, shared=True)), _words(*_solve(f, Sr, torch.zeros_like(Si), n, shared=True)))
    for k in range(K):                                    # and is the shared run of that member alone
        assert np.array_equal(_words(*_solve(f, Sr, Si, n, K=1, first=k, shared=True)), shared[:, :, k * n:(k + 1) * n]), k
    # in place: every member on its own columns; a shared rhs with one member
    for m in (1, n):
        Xr, Xi = Br[:, :K * m].clone(), Bi[:, :K * m].clone()
        want = _words(*_solve(f, Br[:, :K * m].contiguous(), Bi[:, :K * m].contiguous(), m))
        f.solve_complex(Xr.data_ptr(), Xi.data_ptr(), Xr.data_ptr(), Xi.data_ptr(), n_rhs=m)
        torch.cuda.synchronize()
        assert np.array_equal(_words(Xr, Xi), want), m
    Xr, Xi = Sr.clone(), Si.clone()
    f.solve_complex(Xr.data_ptr(), Xi.data_ptr(), Xr.data_ptr(), Xi.data_ptr(), n_rhs=n, first_member=2, n_members=1, shared_rhs=True)
    torch.cuda.synchronize()
    assert np.array_equal(_words(Xr, Xi), shared[:, :, 2 * n:])
    # a second factor
    f2 = _factor(c, alpha, beta)
    assert np.array_equal(_words(*_solve(f2, Br, Bi, n)), ref)
    assert [_info_words(f, k) for k in range(K)] == [_info_words(f2, k) for k in range(K)]
    f2.close()
    # the refusals that read the factor
    import slod_amd
    for kw, word in ((dict(first_member=2, n_members=2), "members outside the factor"), (dict(first_member=-1), "members outside"),
                     (dict(ld_u=K * n - 1), "leading dimension of u"), (dict(ld_rhs=K * n - 1), "rhs below n_members * n_rhs"),
                     (dict(shared_rhs=True, ld_rhs=n - 1), "shared rhs below n_rhs"), (dict(n_rhs=0), "n_rhs < 1")):
        args = dict(n_rhs=n)
        args.update(kw)
        with pytest.raises(slod_amd.SlodError) as e:
            f.solve_complex(Br.data_ptr(), Bi.data_ptr(), ur.data_ptr(), ui.data_ptr(), **args)
        assert e.value.code == -1 and "slod_lod_factor_solve_complex:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    for rhs, u in (((Sr, Si), (Sr, ui)), ((Sr, Si), (ur, Si)), ((Sr, None), (Sr, ui))):
        with pytest.raises(slod_amd.SlodError) as e:
            f.solve_complex(rhs[0].data_ptr(), _ptr(rhs[1]), u[0].data_ptr(), u[1].data_ptr(), n_rhs=n, shared_rhs=True, ld_u=K * n + 7)
        assert e.value.code == -1 and "in place" in str(e.value)
    f.close()


@pytest.mark.parametrize("name,K", [("rowmajor", 3), ("morton16", 3), ("rowmajor", 65), ("s2", 65)])
def test_zldl_members_have_the_words_of_the_one_member_factor(so, name, K):
    c = hc.harmonic_case(so, name)
    dm, ds, freqs = c.sweep["both"]
    if K == 3:
        omegas = np.array([freqs[k][0] for k in (1, 7, 4)])
    else:
        omegas = np.array([w for w, _, _ in _sweep65(c)[2]])
    alpha, beta = hc.coefficients(omegas, dm, ds)
    f = _factor(c, alpha, beta)
    assert (f.bad_pivot == -1).all()
    n = 3
    hb, Br, Bi = _loads(np.random.default_rng(507), c.nrow, n, True)
    wide = _words(*_solve(f, Br, Bi, n, shared=True))
    for k in range(K):
        fk = _factor(c, alpha[k], beta[k])
        assert _info_words(fk, 0) == _info_words(f, k), k
        assert np.array_equal(_words(*_solve(fk, Br, Bi, n, shared=True)), wide[:, :, k * n:(k + 1) * n]), k
        fk.close()
    f.close()


# ---- the real limit

@pytest.mark.parametrize("name", lc.CASES)
def test_real_coefficients_give_the_real_factor(so, name):
    torch, dev = _torch()
    c = hc.harmonic_case(so, name)
    rng = np.random.default_rng(509)
    n = 5
    hb, Br, _ = _loads(rng, c.nrow, n, False)
    for sigma in (0.0, 0.5 * c.lam[0], 2.0 * c.lam[-1]):
        f = _factor(c, [1.0], [-sigma])
        ur, ui = _solve(f, Br, None, n)
        assert bool((ui == 0.0).all()) and bool(torch.isfinite(ur).all())
        values, S = lc.shifted_values(c, sigma)
        fr = c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())
        xr = _nan(c.nrow, n)
        fr.solve(Br.data_ptr(), xr.data_ptr(), n_rhs=n)
        torch.cuda.synchronize()
        got, want = ur.cpu().numpy(), xr.cpu().numpy()
        rel = (np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)).max()
        ri, zi = fr.inertia(), f.inertia()
        print("%s sigma %.6e: complex factor against the real LDL^T %.3e, growth %.3e / %.3e" % (name, sigma, rel, zi.growth, ri.growth))
        assert rel <= 1e-8, (name, sigma, rel)
        assert zi.norm_matrix == ri.norm_matrix and zi.max_abs_pivot == pytest.approx(ri.max_abs_pivot, rel=1e-10)
        zr, zi_ = _solve(f, torch.zeros_like(Br), None, n)
        assert bool((zr == 0.0).all()) and bool((zi_ == 0.0).all())
        zr, zi_ = _solve(f, torch.zeros_like(Br), torch.zeros_like(Br), n)
        assert bool((zr == 0.0).all()) and bool((zi_ == 0.0).all())
        fr.close()
        f.close()


# ---- failure: a status word, not a device fault

def test_zldl_refuses_nan_and_a_zero_member(so):
    import slod_amd
    c = hc.harmonic_case(so, "morton16")
    dm, ds, freqs = c.sweep["both"]
    omegas = np.array([freqs[k][0] for k in (5, 6, 7)])
    alpha, beta = hc.coefficients(omegas, dm, ds)
    cap = c.g.lod_row_capacity()
    hcols = c.cols.cpu().numpy().view(np.uint32).reshape(-1, cap)
    r = int(c.perm[c.nrow // 2])                       # a row in the middle of the band, s = 1: row = patch
    at = {int(row): k for k, row in enumerate(c.perm)}
    under = [j for j in range(cap) if hcols[r, j] != 0xffffffff and at[int(hcols[r, j])] < c.nrow // 2]
    holed = c.sym.clone()
    holed[r * cap + under[0]] = NAN                    # an entry of the lower triangle in factor order
    Ah = c.A.copy()
    Ah[r, int(hcols[r, under[0]])] = NAN               # the yardstick reads the lower triangle in factor order only
    want_nan = [hc.zldl_reference(hc.system(Ah, c.M, w, dm, ds)[np.ix_(c.perm, c.perm)]).bad for w in omegas]
    assert want_nan == [c.nrow // 2] * 3
    a0, b0 = alpha.copy(), beta.copy()
    a0[1] = b0[1] = 0.0
    assert hc.zldl_reference(hc.combined(c.A, c.M, 0.0, 0.0)).bad == 0
    for what, A_t, al, be, want in (("NaN", holed, alpha, beta, want_nan), ("zero member", c.sym, a0, b0, [-1, 0, -1])):
        out, bad = C.c_void_p(1), np.full(3, 7, dtype=np.int32)
        ap, bp = np.ascontiguousarray(al).view(np.float64), np.ascontiguousarray(be).view(np.float64)
        rc = c.g.lib.slod_lod_factor_create_zldl(c.g.h, A_t.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(),
                                                 ap.ctypes.data_as(C.POINTER(C.c_double)), bp.ctypes.data_as(C.POINTER(C.c_double)), 3,
                                                 bad.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(out))
        msg = c.g.lib.slod_last_error(c.g.h).decode()
        print("%s: %d, %s" % (what, rc, msg))
        assert rc == -5 and out.value is None and list(bad) == want, (what, rc, list(bad))
        first = [k for k in range(3) if want[k] >= 0][0]
        m = re.search(r"slod_lod_factor_create_zldl: member (\d+): pivot (\d+) of %d is zero or not finite \((.*), (.*)\)" % c.nrow, msg)
        assert m and (int(m.group(1)), int(m.group(2))) == (first, want[first]), msg
        with pytest.raises(slod_amd.SlodError) as e:
            _factor(c, al, be) if A_t is c.sym else c.g.lod_factor_zldl(A_t.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), al, be)
        assert e.value.code == -5 and list(e.value.bad_pivot) == want
    # the same call without the bad member succeeds, and meets the bound
    f = _factor(c, alpha[[0, 2]], beta[[0, 2]])
    assert (f.bad_pivot == -1).all()
    hb, Br, Bi = _loads(np.random.default_rng(511), c.nrow, 3, True)
    x = _z(*_solve(f, Br, Bi, 3, shared=True))
    for j, k in enumerate((0, 2)):
        ref = freqs[(5, 6, 7)[k]][1]
        e = hc.zeta(hc.system(c.A, c.M, omegas[k], dm, ds), ref.G, x[:, 3 * j:3 * j + 3], hb)
        assert (e <= hc.ZBOUND * hc.bound(c.hbw)).all()
    f.close()


# ---- the sweep call

_sweeps = {}


def _sweep65(c):
    """The rule's eight frequencies and 57 evenly spaced ones at the damping `both`, every one qualified; built once."""
    key = id(c)
    if key not in _sweeps:
        _sweeps[key] = hc.sweep(c.lam_h, c.A, c.M, c.perm, extra=57)["both"]
    return _sweeps[key]


@pytest.mark.parametrize("name", ["rowmajor", "s2"])
def test_harmonic_response_sweep(so, name):
    torch, dev = _torch()
    c = hc.harmonic_case(so, name)
    g = c.g
    dm, ds, freqs = _sweep65(c)
    assert len(freqs) == 65
    moved = [(k, m) for k, (_, _, m) in enumerate(freqs) if m]
    print("%s: %d of 65 frequencies moved %r; worst yardstick growth %.3e" % (name, len(moved), moved, max(r.G / r.norm for _, r, _ in freqs)))
    omegas = np.array([w for w, _, _ in freqs])
    rng = np.random.default_rng(521)
    hb = rng.uniform(-1.0, 1.0, (c.nrow, 3)) + 1j * rng.uniform(-1.0, 1.0, (c.nrow, 3))
    hb[:, 0] = c.M @ c.X[:, 0]                           # the first mode's load, real
    Br, Bi = _dev(hb.real), _dev(hb.imag)
    nearest = int(np.argmin(np.abs(omegas - np.sqrt(c.lam_h[0]))))
    for nf in (1, 8, 65):
        w = omegas[:nf]
        alpha, beta = hc.coefficients(w, dm, ds)
        for n in (1, 3):
            ur, ui = _nan(c.nrow, nf * n + 2), _nan(c.nrow, nf * n + 2)
            res, growth = g.lod_harmonic_response(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), w, Br.data_ptr(),
                                                  Bi.data_ptr() if n > 1 else None, ur.data_ptr(), ui.data_ptr(), n_rhs=n,
                                                  damp_mass=dm, damp_stiff=ds, ld_load=3, ld_u=nf * n + 2)
            assert bool(torch.isnan(ur[:, nf * n:]).all()) and bool(torch.isnan(ui[:, nf * n:]).all())
            assert res.shape == (nf, n) and growth.shape == (nf,)
            load = hb[:, :n] if n > 1 else hb[:, :1].real + 0j
            got = _words(ur[:, :nf * n], ui[:, :nf * n])
            x = _z(ur[:, :nf * n], ui[:, :nf * n])
            for k in range(nf):                              # the words of create_zldl + solve_complex per frequency
                fk = _factor(c, alpha[k], beta[k])
                one = _words(*_solve(fk, Br, Bi if n > 1 else None, n, shared=True))
                assert np.array_equal(one, got[:, :, k * n:(k + 1) * n]), (nf, n, k)
                assert growth[k] == fk.inertia().growth
                fk.close()
                S = hc.system(c.A, c.M, w[k], dm, ds)
                xk = x[:, k * n:(k + 1) * n]
                r = load.astype(np.clongdouble) - S.astype(np.clongdouble) @ xk.astype(np.clongdouble)
                true = np.array(np.sqrt((np.abs(r) ** 2).sum(axis=0)) / np.linalg.norm(load, axis=0), dtype=np.float64)
                room = 64 * hc.U * (np.abs(S).sum(axis=1).max() * np.linalg.norm(xk, axis=0) / np.linalg.norm(load, axis=0) + 1.0)
                assert (np.abs(res[k] - true) <= np.maximum(1e-6 * true, room)).all(), (nf, n, k, res[k], true)
            # the power identity  omega (dm u^H M u + ds u^H A u) = Im(u^H b)  with slod_lod_inner_multi
            ucr, uci = ur[:, :nf * n].contiguous(), ui[:, :nf * n].contiguous()
            quad = {}
            for key, values in (("M", c.mvalues), ("A", c.sym)):
                quad[key] = sum(g.lod_inner(values.data_ptr(), c.cols.data_ptr(), t.data_ptr(), t.data_ptr(), n_rhs=nf * n)
                                for t in (ucr, uci))
            torch.cuda.synchronize()
            ub = np.array([np.vdot(x[:, j], load[:, j % n]) for j in range(nf * n)])
            power = np.repeat(w, n) * (dm * quad["M"] + ds * quad["A"])
            assert (np.abs(power - ub.imag) <= 1e-8 * np.abs(ub)).all(), (nf, n, (np.abs(power - ub.imag) / np.abs(ub)).max())
            if nf == 65:                                     # the transfer function peaks at the first resonance
                amp = np.sqrt(quad["M"][0::n])
                print("%s n_rhs %d: residual <= %.3e, growth <= %.3e, power identity off by %.3e, amplitude peak at sample %d "
                      "(omega %.6e)" % (name, n, res.max(), growth.max(), (np.abs(power - ub.imag) / np.abs(ub)).max(),
                                        int(np.argmax(amp)), w[int(np.argmax(amp))]))
                assert int(np.argmax(amp)) == nearest, (int(np.argmax(amp)), nearest)
    # a zero load column: u = 0 and residual 0
    Z = torch.zeros((c.nrow, 2), dtype=torch.float64, device=dev)
    Z[:, 1] = Br[:, 1]
    ur, ui = _nan(c.nrow, 4), _nan(c.nrow, 4)
    res, _ = g.lod_harmonic_response(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), omegas[:2], Z.data_ptr(), None,
                                     ur.data_ptr(), ui.data_ptr(), n_rhs=2, damp_mass=dm, damp_stiff=ds)
    assert bool((ur[:, 0::2] == 0.0).all()) and bool((ui[:, 0::2] == 0.0).all()) and (res[:, 0] == 0.0).all() and (res[:, 1] > 0.0).all()
    # omega = 0 without damping: S = A, real, the imaginary plane stays exact zeros
    res, growth = g.lod_harmonic_response(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), [0.0], Z.data_ptr(), None,
                                          ur.data_ptr(), ui.data_ptr(), n_rhs=2, ld_u=4)
    want = np.linalg.solve(c.A, Z.cpu().numpy())
    assert bool((ui[:, :2] == 0.0).all()) and np.abs(ur[:, :2].cpu().numpy() - want).max() <= 1e-8 * np.abs(want).max()


def test_harmonic_response_reports_the_failed_frequency(so):
    import slod_amd
    torch, dev = _torch()
    c = hc.harmonic_case(so, "rowmajor")
    Z = c.mvalues * 0.0
    ur, ui, B = _nan(c.nrow, 3), _nan(c.nrow, 3), _dev(np.ones((c.nrow, 1)))
    with pytest.raises(slod_amd.SlodError) as e:         # A = M = 0: every pivot of every frequency is zero
        c.g.lod_harmonic_response(Z.data_ptr(), Z.data_ptr(), c.cols.data_ptr(), [1.0, 2.0, 3.0], B.data_ptr(), None, ur.data_ptr(),
                                  ui.data_ptr(), damp_mass=0.1)
    assert e.value.code == -5 and "slod_lod_harmonic_response: frequency 0: pivot 0 of %d is zero or not finite (0, 0)" % c.nrow in str(e.value)
    res, growth = c.g.lod_harmonic_response(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), [1.0, 2.0, 3.0], B.data_ptr(), None,
                                            ur.data_ptr(), ui.data_ptr(), damp_mass=0.1)
    assert np.isfinite(res).all() and bool(torch.isfinite(ur).all())


# ---- every other consumer of a factor refuses a complex one; the complex solve refuses a real one

def test_consumers_refuse_the_other_kind_of_factor(so):
    import slod_amd
    torch, dev = _torch()
    c = hc.harmonic_case(so, "rowmajor")
    g = c.g
    f = _factor(c, [1.0 + 0.1j], [-1.0 + 0.2j])
    text = "a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex"
    U0, V0, A0 = (_dev(np.ones((c.nrow, 1))) for _ in range(3))
    X = _nan(c.nrow, 8)
    sym, mass, cols = c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr()
    calls = {
        "slod_lod_factor_solve": lambda: g._check(g.lib.slod_lod_factor_solve(f.f, U0.data_ptr(), 1, 1, V0.data_ptr(), 1, None)),
        "slod_lod_factor_solve_ensemble": lambda: slod_amd.EnsembleFactor.solve(f, U0.data_ptr(), V0.data_ptr()),
        "slod_lod_theta_steps_direct": lambda: g.lod_theta_steps_direct(f, sym, cols, 0.01, 0.5, 1, U0.data_ptr()),
        "slod_lod_newmark_accel_direct": lambda: g.lod_newmark_accel_direct(f, sym, mass, cols, U0.data_ptr(), V0.data_ptr(), A0.data_ptr()),
        "slod_lod_newmark_steps_direct": lambda: g.lod_newmark_steps_direct(f, sym, mass, cols, 0.01, 1, U0.data_ptr(), V0.data_ptr(),
                                                                            A0.data_ptr()),
        "slod_lod_eigs_direct": lambda: g.lod_eigs_direct(f, sym, mass, cols, 2, X.data_ptr(), n_block=8),
        "slod_lod_eigs_shift_direct": lambda: g.lod_eigs_shift_direct(f, 1.0, sym, mass, cols, 2, X.data_ptr(), n_block=8),
        "slod_lod_solve_multi_precond": lambda: g.lod_solve_multi_precond(f, sym, cols, U0.data_ptr(), 1, 1, V0.data_ptr(), 1),
    }
    for who, call in calls.items():
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith(who + ": " + text), (who, str(e.value))
    assert bool((U0 == 1.0).all()) and bool((V0 == 1.0).all())
    f.close()
    for real in (g.lod_factor(c.sym.data_ptr(), cols), g.lod_factor_ldl(c.sym.data_ptr(), cols)):
        rc = g.lib.slod_lod_factor_solve_complex(real.f, 0, 1, U0.data_ptr(), None, 1, 1, 0, V0.data_ptr(), A0.data_ptr(), 1, None)
        msg = g.lib.slod_last_error(g.h).decode()
        assert rc == -1 and msg.startswith("slod_lod_factor_solve_complex: a real factor") and "slod_lod_factor_solve" in msg, msg
        real.close()


# ---- the mirror and the driver

def test_driver_harmonic_matches_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --harmonic 5 W0 W1 --damping DM DS (the driver's coefficient Alpha(1, 100, 3), srand(1);
    f = 1) prints per frequency the growth, the residual, the amplitude and the dissipated power of the Python path, to
    the digits printed."""
    import os
    import subprocess
    from lod_cases import _build, _mass, _symmetrize
    torch, dev = _torch()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "dealii-slod_amd", "bin", "main_Diffusion")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", os.path.join(root, "dealii-slod_amd"), "bin/main_Diffusion"])
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    g = c.g
    c.mvalues, _ = _mass(c)
    c.sym = _symmetrize(c)
    from lod_cases import _rows_to_dense
    import scipy.linalg as sl
    hcols = c.cols.cpu().numpy().view(np.uint32)
    lam = sl.eigh(_rows_to_dense(g, c.sym.cpu().numpy(), hcols, 1), _rows_to_dense(g, c.mvalues.cpu().numpy(), hcols, 1),
                  eigvals_only=True)
    w1 = float(np.sqrt(lam[0]))
    K, w0, wK, dm, ds = 5, 0.5 * w1, 2.0 * w1, 0.02 * w1, 1e-3 / w1
    r = subprocess.run([binary, "3", "4", "1", "1", "--harmonic", str(K), repr(w0), repr(wK), "--damping", repr(dm), repr(ds)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"^harmonic (\d+): omega = (\S+), growth = (\S+), relative residual = (\S+), amplitude = (\S+), power = (\S+)$",
                       r.stdout, re.M)
    assert [int(m[0]) for m in lines] == list(range(1, K + 1)), r.stdout
    # the Python path, the driver's frequencies
    omegas = np.array([w0 + k * ((wK - w0) / (K - 1)) for k in range(K)])
    f = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, f.data_ptr())
    rhs = torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
    g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, f.data_ptr(), rhs.data_ptr())
    ur, ui = _nan(c.nrow, K), _nan(c.nrow, K)
    res, growth = g.lod_harmonic_response(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), omegas, rhs.data_ptr(), None,
                                          ur.data_ptr(), ui.data_ptr(), damp_mass=dm, damp_stiff=ds)
    uMu = sum(g.lod_inner(c.mvalues.data_ptr(), c.cols.data_ptr(), t.data_ptr(), t.data_ptr(), n_rhs=K) for t in (ur, ui))
    uAu = sum(g.lod_inner(c.sym.data_ptr(), c.cols.data_ptr(), t.data_ptr(), t.data_ptr(), n_rhs=K) for t in (ur, ui))
    amp, power = np.sqrt(uMu), 0.5 * omegas * (dm * uMu + ds * uAu)
    for k, m in enumerate(lines):
        want = ("%.12e" % omegas[k], "%.6e" % growth[k], "%.6e" % res[k, 0], "%.12e" % amp[k], "%.12e" % power[k])
        assert tuple(m[1:]) == want, (k, m, want)
    assert int(np.argmax(amp)) == int(np.argmin(np.abs(omegas - w1)))
