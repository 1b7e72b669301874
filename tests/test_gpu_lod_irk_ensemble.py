"""GPU tests of the two-stage implicit Runge-Kutta steppers on a coefficient ensemble
(slod_lod_irk_heat_steps_ensemble_direct, slod_lod_irk_wave_steps_ensemble_direct): a matrix, a member of the complex
factor and a column per member.  Every comparison is one of 64-bit words against the single call
(slod_lod_irk_heat_steps_direct, slod_lod_irk_wave_steps_direct with n_rhs = 1) on the de-interleaved member and its own
one-member factor unless it says otherwise.

Configurations, time steps, dampings and loads: lod_irk_ensemble_cases.py (the three configurations of
test_gpu_lod_ensemble_wave.py, K = 3 and on base K = 65; the rule of lod_irk_cases.py on the joint spectrum).  3 steps
unless stated.

Bars that are not equality of words:
  yardstick     1e-8 of max |reference| per member against the undiagonalised stage system of lod_irk_cases.py on the
                member's dense pencil (FORWARD, the project's bar against a dense reference); the growth cap is asserted on
                the yardstick of every member before the library is called
  conservation  Gauss, undamped, 10 steps at dt = 0.7 / omega_1: relative energy drift <= 1e-8 per member
  decay         with damping no step raises the energy beyond 1e-12 of its value; Radau heat at dt = 10 / lambda_1:
                u_m^T M_m u_m falls every step
  driver        the per-member lines agree to the digits printed; |kinetic + potential - work| <= 1e-8 max potential
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_irk_cases as ic
import lod_irk_ensemble_cases as ec
from lod_cases import _bits, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
STEPS = 3
PROBLEMS = ("heat", "wave-none", "wave-mass", "wave-stiff", "wave-both")
REFUSED = "takes a complex factor (slod_lod_factor_create_zldl)"
PADS = (1, 2, 3)      # of u, v and the load in the padded runs; the matrices: ld_a_m = K + 1, ld_m_m = K + 2


def _problem(c, label):
    return next(p for p in ec.problems(c.lam) if p[0] == label)


def _data(c, K, seed, steps=STEPS):
    """A state (u, v) per member, a constant load and stage loads (lod_irk_cases.stage_loads), per member."""
    rng = np.random.default_rng(seed)
    u0 = rng.uniform(-1.0, 1.0, (c.nrow, K))
    v0 = np.sqrt(c.lam[0][c.nrow // 2]) * rng.uniform(-1.0, 1.0, (c.nrow, K))
    const = ic.stage_loads(rng, 1, (c.nrow, K))[0]
    stage = ic.stage_loads(rng, steps, (c.nrow, K))
    return u0, v0, {"none": None, "constant": const, "stage": stage}


def _matrices(c, K, pad=True):
    return ec.stack(c, c.sym, K, pad=1 if pad else 0), ec.stack(c, c.mass, K, pad=2 if pad else 0)


def _ens_factor(c, A, M, K, scheme, order, dts, dm=0.0, ds=0.0):
    """Factor member k K + m: dt_k on member m."""
    torch, _ = _torch()
    pairs = [c.g.lod_irk_coefficients(scheme, order, dt, dm, ds) for dt in np.atleast_1d(dts)]
    torch.cuda.synchronize()
    f = c.g.lod_factor_zldl_ensemble(A.data_ptr(), M.data_ptr(), c.cols.data_ptr(), K, [p[0] for p in pairs],
                                     [p[1] for p in pairs], ld_a_m=A.shape[1], ld_b_m=M.shape[1])
    assert (f.bad_pivot == -1).all() and f.n_members == len(pairs) * K
    return f


def _one_factor(c, Ak, Mk, scheme, order, dt, dm=0.0, ds=0.0):
    a, b = c.g.lod_irk_coefficients(scheme, order, dt, dm, ds)
    return c.g.lod_factor_zldl(Ak.data_ptr(), Mk.data_ptr(), c.cols.data_ptr(), [a], [b])


def _load_args(loads, K, pad):
    """(tensor kept alive, d_load, ld_load, stride) for None, a constant [rows][K] or stage loads [2 steps][rows][K]."""
    if loads is None:
        return None, None, K, 0
    t = ec.padded(loads, pad)
    return t, t.data_ptr(), K + pad, 0 if loads.ndim == 2 else loads.shape[1] * (K + pad)


def _ens(c, f, first, scheme, order, A, M, dt, dm, ds, steps, u0, v0, loads, pads=(0, 0, 0), energies=True, offset=0, K=None):
    """The ensemble call on fresh device copies; returns (U, V, kinetic, potential, load tensor).  offset: members skipped
    at the front of every array by pointer offset (a member sub-range)."""
    torch, _ = _torch()
    g, cols = c.g, c.cols.data_ptr()
    K = u0.shape[1] - offset if K is None else K
    U, V = ec.padded(u0, pads[0]), ec.padded(v0, pads[1])
    L, d_load, ld_load, stride = _load_args(loads, u0.shape[1], pads[2])
    o = 8 * offset
    torch.cuda.synchronize()
    if order == 1:
        g.lod_irk_heat_steps_ensemble(f, scheme, A.data_ptr() + o, cols, dt, steps, K, U.data_ptr() + o, first_member=first,
                                      ld_a_m=A.shape[1], ld_u=U.shape[1], d_load=None if d_load is None else d_load + o,
                                      ld_load=ld_load, load_stage_stride=stride)
        kin = pot = None
    else:
        kin, pot = g.lod_irk_wave_steps_ensemble(f, scheme, A.data_ptr() + o, M.data_ptr() + o, cols, dt, steps, K, U.data_ptr() + o,
                                                 V.data_ptr() + o, first_member=first, ld_a_m=A.shape[1], ld_m_m=M.shape[1],
                                                 ld_u=U.shape[1], ld_v=V.shape[1], d_load=None if d_load is None else d_load + o,
                                                 ld_load=ld_load, load_stage_stride=stride, damp_mass=dm, damp_stiff=ds,
                                                 energies=energies)
    torch.cuda.synchronize()
    return U, V, kin, pot, L


def _single(c, fk, scheme, order, Ak, Mk, dt, dm, ds, steps, u0k, v0k, loadk, member=0):
    """The single call with n_rhs = 1 on one member; returns the words of u and v and the energies' columns."""
    torch, _ = _torch()
    g, cols = c.g, c.cols.data_ptr()
    u, v = ec.dev(u0k[:, None]), ec.dev(v0k[:, None])
    keep = None if loadk is None else ec.dev(loadk)
    d_load = None if keep is None else keep.data_ptr()
    stride = 0 if loadk is None or loadk.ndim == 1 else c.nrow
    torch.cuda.synchronize()
    if order == 1:
        g.lod_irk_heat_steps(fk, scheme, Ak.data_ptr(), cols, dt, steps, u.data_ptr(), member=member, d_load=d_load,
                             load_stage_stride=stride)
        kin = pot = None
    else:
        kin, pot = g.lod_irk_wave_steps(fk, scheme, Ak.data_ptr(), Mk.data_ptr(), cols, dt, steps, u.data_ptr(), v.data_ptr(),
                                        member=member, d_load=d_load, load_stage_stride=stride, damp_mass=dm, damp_stiff=ds)
    torch.cuda.synchronize()
    return _bits(u)[:, 0], _bits(v)[:, 0], kin, pot


def _words(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_words(a), _words(b))


def _nan_padding(*pairs):
    for t, n in pairs:
        if t is not None:
            assert bool(t[..., n:].isnan().all())


# ---- 1. words against the single calls

@pytest.mark.parametrize("problem", PROBLEMS)
@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
@pytest.mark.parametrize("name,K", ec.CASES)
def test_ensemble_words_equal_the_single_calls(so, name, K, label, scheme, problem):
    c = ec.ens_case(so, name)
    _, order, dts, dm, ds = _problem(c, problem)
    u0, v0, loads = _data(c, K, 801)
    A, M = _matrices(c, K)                                             # ld_a_m = K + 1, ld_m_m = K + 2
    f = _ens_factor(c, A, M, K, scheme, order, dts, dm, ds)
    members = [(A[:, k].contiguous(), M[:, k].contiguous()) for k in range(K)]
    for m, dt in enumerate(dts):
        singles = [_one_factor(c, Ak, Mk, scheme, order, dt, dm, ds) for Ak, Mk in members]
        for kind, b in loads.items():
            U, V, kin, pot, L = _ens(c, f, m * K, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b, pads=PADS)
            _nan_padding((U, K), (V, K), (L, K))
            Ub, Vb = _bits(U[:, :K]), _bits(V[:, :K])
            assert np.isfinite(U[:, :K].cpu().numpy()).all()
            if order == 2:
                assert kin.shape == pot.shape == (STEPS + 1, K) and np.isfinite(kin).all() and np.isfinite(pot).all()
                # the energies change no state
                U2, V2, k2, p2, _ = _ens(c, f, m * K, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b, pads=PADS, energies=False)
                assert (k2, p2) == (None, None)
                assert np.array_equal(_bits(U2[:, :K]), Ub) and np.array_equal(_bits(V2[:, :K]), Vb)
            for k in range(K):
                bk = None if b is None else np.ascontiguousarray(b[..., k])
                Ak, Mk = members[k]
                su, sv, sk, sp = _single(c, singles[k], scheme, order, Ak, Mk, dt, dm, ds, STEPS, u0[:, k], v0[:, k], bk)
                where = (name, K, label, problem, m, kind, k)
                assert np.array_equal(Ub[:, k], su), where
                if order == 2:
                    assert np.array_equal(Vb[:, k], sv), where
                    assert _same(kin[:, k], sk[:, 0]) and _same(pot[:, k], sp[:, 0]), where
        for fk in singles:
            fk.close()
    _nan_padding((A, K), (M, K))
    f.close()


# ---- 2. layout

@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
@pytest.mark.parametrize("name,K", ec.CASES)
def test_layout_does_not_change_the_words(so, name, K, label, scheme):
    torch, dev = _torch()
    c = ec.ens_case(so, name)
    u0, v0, loads = _data(c, K, 803)
    stage = loads["stage"][:4]
    A, M = _matrices(c, K, pad=False)
    Ap, Mp = _matrices(c, K)
    for problem in ("heat", "wave-both"):
        _, order, dts, dm, ds = _problem(c, problem)
        dt = dts[1] if order == 1 else dts[0]
        f = _ens_factor(c, A, M, K, scheme, order, dt, dm, ds)

        def run(steps=2, b=stage, u=u0, v=v0, **kw):
            U, V, kin, pot, L = _ens(c, kw.pop("f", f), 0, scheme, order, kw.pop("A", A), kw.pop("M", M), dt, dm, ds, steps, u, v, b, **kw)
            return U, V, kin, pot, L

        U, V, kin, pot, _ = run()
        ref = [_bits(U), _bits(V), _words(kin), _words(pot)]

        def check(got, n=K, cols=slice(None)):
            Ug, Vg, kg, pg, Lg = got
            assert np.array_equal(_bits(Ug[:, :n]), ref[0][:, cols]) and np.array_equal(_bits(Vg[:, :n]), ref[1][:, cols])
            if order == 2:
                assert np.array_equal(_words(kg), ref[2][:, cols]) and np.array_equal(_words(pg), ref[3][:, cols])
            _nan_padding((Ug, n), (Vg, n), (Lg, n))

        check(run())                                                   # a repeated call
        fp = _ens_factor(c, Ap, Mp, K, scheme, order, dt, dm, ds)      # padded everywhere, ld_a_m != ld_m_m
        check(run(f=fp, A=Ap, M=Mp, pads=PADS))
        check(run(f=fp, A=Ap, M=Mp, pads=(3, 1, 2)))
        _nan_padding((Ap, K), (Mp, K))
        fp.close()
        # n_steps = 2 is two calls with n_steps = 1, the second on the loads of the second step
        Ua, Va, ka, pa, _ = run(steps=1, b=stage[:2])
        Ub, Vb, kb, pb, _ = run(steps=1, b=stage[2:], u=Ua.cpu().numpy(), v=Va.cpu().numpy())
        assert np.array_equal(_bits(Ub), ref[0]) and np.array_equal(_bits(Vb), ref[1])
        if order == 2:
            assert _same(np.concatenate([ka, kb[1:]]), kin) and _same(np.concatenate([pa, pb[1:]]), pot) and _same(ka[1], kb[0])
        # permuted members give permuted columns
        perm = np.random.default_rng(804).permutation(K)
        tp = torch.from_numpy(perm).to(dev)
        Aq, Mq = A[:, tp].contiguous(), M[:, tp].contiguous()
        fq = _ens_factor(c, Aq, Mq, K, scheme, order, dt, dm, ds)
        check(run(f=fq, A=Aq, M=Mq, b=stage[:, :, perm], u=u0[:, perm], v=v0[:, perm]), cols=perm)
        fq.close()
        f.close()


# ---- 3. several dt in one object

@pytest.mark.parametrize("name,K", ec.CASES)
def test_several_dt_in_one_factor_and_member_sub_ranges(so, name, K):
    c = ec.ens_case(so, name)
    u0, v0, loads = _data(c, K, 805)
    b = loads["stage"]
    A, M = _matrices(c, K, pad=False)
    for label, scheme in ic.SCHEMES:
        for problem in ("heat", "wave-both"):
            _, order, dts, dm, ds = _problem(c, problem)
            f2 = _ens_factor(c, A, M, K, scheme, order, dts[:2], dm, ds)
            f1 = _ens_factor(c, A, M, K, scheme, order, dts[1], dm, ds)
            assert (f2.n_members, f1.n_members) == (2 * K, K)
            dt = dts[1]
            want = _ens(c, f1, 0, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b)
            full = _ens(c, f2, K, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b)
            other = _ens(c, f2, 0, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b)    # dt_0's factor: other words
            for i in range(4):
                assert _same(_bits(full[i]) if i < 2 else full[i], _bits(want[i]) if i < 2 else want[i]), (label, problem, i)
            assert not np.array_equal(_bits(other[0]), _bits(want[0]))
            # members 1 .. K - 1 by pointer offset: first_member = K + 1 is no multiple of n_members = K - 1
            sub = _ens(c, f2, K + 1, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b, offset=1)
            assert np.array_equal(_bits(sub[0])[:, 1:], _bits(full[0])[:, 1:]), (label, problem)
            assert np.array_equal(_bits(sub[0])[:, 0], _bits(ec.dev(u0))[:, 0])          # member 0 was not touched
            if order == 2:
                assert np.array_equal(_bits(sub[1])[:, 1:], _bits(full[1])[:, 1:])
                assert np.array_equal(_bits(sub[1])[:, 0], _bits(ec.dev(v0))[:, 0])
                assert _same(sub[2], full[2][:, 1:]) and _same(sub[3], full[3][:, 1:])
            f1.close()
            f2.close()


# ---- 4. against the yardstick

@pytest.mark.parametrize("name", ec.NAMES)
def test_members_against_the_stage_system(so, name):
    c = ec.ens_case(so, name)
    K = c.K
    u0, v0, loads = _data(c, K, 807)
    b = loads["stage"]
    A, M = _matrices(c, K, pad=False)
    worst, growth = {}, 0.0
    for label, scheme in ic.SCHEMES:
        for plabel, order, dts, dm, ds in ec.problems(c.lam):
            for dt in dts:                                             # the condition first, for every member and dt
                for k in range(K):
                    gy, _ = ic.growth(c.dA[k], c.dM[k], scheme, order, dt, dm, ds, c.perm)
                    growth = max(growth, gy)
                    assert gy <= ic.GROWTH_CAP, (name, label, plabel, dt, k, gy)
            f = _ens_factor(c, A, M, K, scheme, order, dts, dm, ds)
            for m, dt in enumerate(dts):
                U, V, kin, pot, _ = _ens(c, f, m * K, scheme, order, A, M, dt, dm, ds, STEPS, u0, v0, b)
                gu, gv = U.cpu().numpy(), V.cpu().numpy()
                assert np.isfinite(gu).all() and np.isfinite(gv).all()
                for k in range(K):
                    if order == 1:
                        ru = ic.heat_stage(c.dA[k], c.dM[k], scheme, dt, STEPS, u0[:, k], b[:, :, k])[-1]
                        errs = {"heat": float(np.abs(gu[:, k] - ru).max() / np.abs(ru).max())}
                    else:
                        ru, rv = ic.wave_stage(c.dA[k], c.dM[k], scheme, dt, STEPS, u0[:, k], v0[:, k], dm, ds, b[:, :, k])
                        rk = 0.5 * np.einsum("ki,ij,kj->k", rv, c.dM[k], rv)
                        rp = 0.5 * np.einsum("ki,ij,kj->k", ru, c.dA[k], ru)
                        errs = {"u": float(np.abs(gu[:, k] - ru[-1]).max() / np.abs(ru[-1]).max()),
                                "v": float(np.abs(gv[:, k] - rv[-1]).max() / np.abs(rv[-1]).max()),
                                "E": float(max(np.abs(kin[:, k] - rk).max(), np.abs(pot[:, k] - rp).max()) / rp.max())}
                    for key, e in errs.items():
                        worst[label, key] = max(worst.get((label, key), 0.0), e)
                        assert e <= ic.FORWARD, (name, label, plabel, m, k, key, e)
            f.close()
    print("%s ensemble, %d steps: growth <= %.3f; worst error of a member against the stage system (heat; wave u, v, energies): "
          "gauss %.3e; %.3e %.3e %.3e, radau %.3e; %.3e %.3e %.3e"
          % (name, STEPS, growth, *[worst[l, k] for l in ("gauss", "radau") for k in ("heat", "u", "v", "E")]))


# ---- 5. physics per member

@pytest.mark.parametrize("name,K", ec.CASES)
def test_gauss_conserves_and_damping_dissipates_per_member(so, name, K):
    c = ec.ens_case(so, name)
    steps = 10
    l1 = ec.joint_spectrum(c.lam)[0]
    dt = 0.7 / np.sqrt(l1)
    u0 = np.random.default_rng(809).uniform(-1.0, 1.0, (c.nrow, K))
    v0 = np.zeros_like(u0)
    A, M = _matrices(c, K, pad=False)
    f = _ens_factor(c, A, M, K, ic.GAUSS, 2, dt)
    _, _, kin, pot, _ = _ens(c, f, 0, ic.GAUSS, 2, A, M, dt, 0.0, 0.0, steps, u0, v0, None)
    f.close()
    E = kin + pot
    assert (kin[0] == 0.0).all() and (E[0] > 0.0).all()
    for k in range(K):
        Ak, _ = ec.member_dense(c, K, k)
        assert E[0, k] == pytest.approx(0.5 * float(u0[:, k] @ Ak @ u0[:, k]), rel=1e-12)
    drift = np.abs(E - E[0]).max(axis=0) / E[0]
    rise = 0.0
    for dlabel, dm, ds in ec.wave_dampings(c.lam)[1:]:
        f = _ens_factor(c, A, M, K, ic.GAUSS, 2, dt, dm, ds)
        _, _, kin, pot, _ = _ens(c, f, 0, ic.GAUSS, 2, A, M, dt, dm, ds, steps, u0, v0, None)
        f.close()
        Ed = kin + pot
        rise = max(rise, float(((Ed[1:] - Ed[:-1]) / Ed[:-1]).max()))
        assert (Ed[1:] <= Ed[:-1] * (1.0 + 1e-12)).all(), (name, K, dlabel)
        assert (Ed[-1] < Ed[0]).all()
    print("%s K = %d Gauss, %d steps at dt = 0.7 / omega_1: largest relative energy drift of a member undamped %.3e; largest "
          "relative rise with damping %.3e" % (name, K, steps, float(drift.max()), rise))
    assert (drift <= 1e-8).all(), drift


@pytest.mark.parametrize("name,K", ec.CASES)
def test_radau_heat_lowers_the_mass_norm_of_every_member(so, name, K):
    torch, dev = _torch()
    c = ec.ens_case(so, name)
    g, cols = c.g, c.cols.data_ptr()
    dt = 10.0 / ec.joint_spectrum(c.lam)[0]
    u0 = np.random.default_rng(811).uniform(-1.0, 1.0, (c.nrow, K))
    A, M = _matrices(c, K, pad=False)
    f = _ens_factor(c, A, M, K, ic.RADAU, 1, dt)
    U = ec.dev(u0)
    torch.cuda.synchronize()
    norms = [g.lod_inner_ensemble(M.data_ptr(), cols, U.data_ptr(), U.data_ptr(), K)]
    for _ in range(3):
        g.lod_irk_heat_steps_ensemble(f, ic.RADAU, A.data_ptr(), cols, dt, 1, K, U.data_ptr())
        norms.append(g.lod_inner_ensemble(M.data_ptr(), cols, U.data_ptr(), U.data_ptr(), K))
    f.close()
    norms = np.array(norms)
    print("%s K = %d Radau heat, dt = 10 / lambda_1: u^T M u of member 0 %s" % (name, K, " ".join("%.3e" % x for x in norms[:, 0])))
    assert (norms[0] > 0.0).all() and (np.diff(norms, axis=0) < 0.0).all(), norms


# ---- 6. refusals that need a factor

def test_ensemble_irk_refusals_that_need_a_factor(so):
    import slod_amd
    torch, dev = _torch()
    c = ec.ens_case(so, "rowmajor")
    g, K, cols = c.g, c.K, c.cols.data_ptr()
    A, M = _matrices(c, K, pad=False)
    U0, V0 = (ec.dev(np.ones((c.nrow, K))) for _ in range(2))
    dt = ec.wave_dts(c.lam)[0]
    heat, wave = "slod_lod_irk_heat_steps_ensemble_direct", "slod_lod_irk_wave_steps_ensemble_direct"
    new = {heat: lambda f, n=K, **kw: g.lod_irk_heat_steps_ensemble(f, "radau", A.data_ptr(), cols, dt, 1, n, U0.data_ptr(),
                                                                     **dict(dict(ld_a_m=K, ld_u=K), **kw)),
           wave: lambda f, n=K, **kw: g.lod_irk_wave_steps_ensemble(f, "gauss", A.data_ptr(), M.data_ptr(), cols, dt, 1, n,
                                                                     U0.data_ptr(), V0.data_ptr(),
                                                                     **dict(dict(ld_a_m=K, ld_m_m=K, ld_u=K, ld_v=K), **kw))}

    def refused(call, text):
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith(text), (text, str(e.value))

    torch.cuda.synchronize()
    # a real factor, single or of K members
    S = ec.nan(c.nval, K)
    g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), dt, A.data_ptr(), K, S.data_ptr())
    torch.cuda.synchronize()
    for real in (g.lod_factor(c.mass[0].data_ptr(), cols), g.lod_factor_ldl(c.sym[0].data_ptr(), cols),
                 g.lod_factor_ensemble(S.data_ptr(), cols, K)):
        for who, call in new.items():
            refused(lambda: call(real), who + ": " + REFUSED)
        real.close()
    z = _ens_factor(c, A, M, K, ic.GAUSS, 2, [dt, 2.0 * dt])          # 2 K members
    for who, call in new.items():
        for first, n in ((-1, K), (K + 1, K), (2 * K, 1), (1, 2 * K)):
            lds = dict(ld_a_m=2 * K, ld_m_m=2 * K, ld_u=2 * K, ld_v=2 * K) if n > K else {}
            if who == heat:
                lds.pop("ld_m_m", None), lds.pop("ld_v", None)
            refused(lambda: call(z, n, first_member=first, **lds), who + ": members outside the factor")
        refused(lambda: call(z, 0), who + ": n_steps < 1 or n_members < 1")
        for ld in ("ld_a_m", "ld_u") + (("ld_m_m", "ld_v") if who == wave else ()):
            refused(lambda: call(z, **{ld: K - 1}), who + ": leading dimension below n_members")
        refused(lambda: call(z, d_load=U0.data_ptr(), ld_load=K - 1), who + ": leading dimension below n_members")
        refused(lambda: call(None), who + ": NULL factor")
    # the factor of another handle
    other = ec.ens_case(so, "base")
    refused(lambda: other.g.lod_irk_heat_steps_ensemble(z, "radau", A.data_ptr(), cols, dt, 1, K, U0.data_ptr()),
            heat + ": factor of another handle / row count")
    refused(lambda: other.g.lod_irk_wave_steps_ensemble(z, "gauss", A.data_ptr(), M.data_ptr(), cols, dt, 1, K, U0.data_ptr(),
                                                        V0.data_ptr()), wave + ": factor of another handle / row count")
    # the real consumers go on refusing the complex factor of several members
    text = "a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex"
    A0 = ec.dev(np.ones((c.nrow, K)))
    old = {"slod_lod_theta_steps_direct": lambda: g.lod_theta_steps_direct(z, c.sym[0].data_ptr(), cols, dt, 0.5, 1, U0.data_ptr(),
                                                                           ld_u=K),
           "slod_lod_newmark_steps_direct": lambda: g.lod_newmark_steps_direct(z, c.sym[0].data_ptr(), c.mass[0].data_ptr(), cols, dt,
                                                                               1, U0.data_ptr(), V0.data_ptr(), A0.data_ptr(),
                                                                               ld_u=K, ld_v=K, ld_a=K),
           "slod_lod_newmark_steps_ensemble_direct": lambda: g.lod_newmark_steps_ensemble_direct(
               z, A.data_ptr(), M.data_ptr(), cols, dt, 1, K, U0.data_ptr(), V0.data_ptr(), A0.data_ptr())}
    for who, call in old.items():
        refused(call, who + ": " + text)
    torch.cuda.synchronize()
    # no device work on a refusal: the states are untouched
    assert bool((U0 == 1.0).all()) and bool((V0 == 1.0).all()) and bool((A0 == 1.0).all())
    # the single calls go on taking `member` of a factor of several members: member K + 1 is dt_1 on member 1
    u0, v0, loads = _data(c, K, 813)
    Ak, Mk = A[:, 1].contiguous(), M[:, 1].contiguous()
    f1 = _one_factor(c, Ak, Mk, ic.GAUSS, 2, 2.0 * dt)
    want = _single(c, f1, ic.GAUSS, 2, Ak, Mk, 2.0 * dt, 0.0, 0.0, STEPS, u0[:, 1], v0[:, 1], None)
    got = _single(c, z, ic.GAUSS, 2, Ak, Mk, 2.0 * dt, 0.0, 0.0, STEPS, u0[:, 1], v0[:, 1], None, member=K + 1)
    for a, b in zip(want, got):
        assert _same(a, b)
    f1.close()
    z.close()


# ---- 7. end to end

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


def test_irk_wave_pipeline_equals_three_single_pipelines(so):
    torch, dev = _torch()
    c = ec.ens_case(so, "base")
    g, K, steps = c.g, c.K, 4
    dt = ec.wave_dts(c.lam)[0]
    V, M, A = ec.nan(c.nval, K), ec.nan(c.nval, K), ec.nan(c.nval, K)
    cols, mcols = torch.zeros_like(c.cols), torch.zeros_like(c.cols)
    R, fine = ec.nan(c.nrow, K), ec.nan(K, c.field)
    Ut, Vt = (torch.zeros(c.nrow, K, dtype=torch.float64, device=dev) for _ in range(2))
    mean, var = ec.nan(c.field), ec.nan(c.field)
    torch.cuda.synchronize()
    g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix_ensemble(c.b.data_ptr(), c.stride, K, M.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, A.data_ptr())
    g.lod_rhs_ensemble(c.b.data_ptr(), c.stride, K, c.load.data_ptr(), R.data_ptr())
    torch.cuda.synchronize()
    alpha, beta = g.lod_irk_coefficients("gauss", 2, dt)
    f = g.lod_factor_zldl_ensemble(A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, [alpha], [beta])
    kin, pot = g.lod_irk_wave_steps_ensemble(f, "gauss", A.data_ptr(), M.data_ptr(), cols.data_ptr(), dt, steps, K, Ut.data_ptr(),
                                             Vt.data_ptr(), d_load=R.data_ptr())
    g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, K, Ut.data_ptr(), fine.data_ptr())
    g.ensemble_moments(fine.data_ptr(), K, c.field, mean.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(cols, c.cols) and torch.equal(mcols, c.cols)
    single = []
    for k in range(K):
        fk = g.lod_factor_zldl(c.sym[k].data_ptr(), c.mass[k].data_ptr(), c.cols.data_ptr(), [alpha], [beta])
        u, v = (torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        k1, p1 = g.lod_irk_wave_steps(fk, "gauss", c.sym[k].data_ptr(), c.mass[k].data_ptr(), c.cols.data_ptr(), dt, steps,
                                      u.data_ptr(), v.data_ptr(), d_load=c.rhs[k].data_ptr())
        out = ec.nan(c.field)
        g.lod_reconstruct(c.slab[k][0].data_ptr(), c.stride, u.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Ut[:, k]), _bits(u[:, 0])) and np.array_equal(_bits(Vt[:, k]), _bits(v[:, 0])), k
        assert _same(kin[:, k], k1[:, 0]) and _same(pot[:, k], p1[:, 0]), k
        single.append(out.cpu().numpy())
        fk.close()
    single = np.stack(single)
    assert np.array_equal(_bits(fine), single.view(np.uint64))
    m, v = _moments_numpy(single)
    assert np.array_equal(_bits(mean), m.view(np.uint64)) and np.array_equal(_bits(var), v.view(np.uint64))
    assert np.isfinite(single).all() and v.max() > 0.0 and np.abs(m).max() > 0.0 and (kin[1:] > 0.0).all()
    f.close()


# ---- 8. the driver

def _driver(*args):
    """A fresh child process per run, under its own time limit."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "2", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


GROWTH_LINE = r"^factor: complex LDL\^T of the (\S+) step, growth = (\S+)$"


def test_driver_ensemble_irk_wave():
    """main_Diffusion 3 2 1 1 --ensemble 3 --wave 4 DT --irk gauss: the lines of member m are those of a single
    --member m --wave 4 DT --irk gauss run, to the digits printed; Gauss keeps kinetic + potential - work = 0 from rest under
    a constant load."""
    K, steps, dt = 3, 4, "0.005"
    out = _driver("--ensemble", str(K), "--wave", str(steps), dt, "--irk", "gauss")
    lines = re.findall(r"^member (\d+) irk wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", out, re.M)
    assert [(int(a), int(b)) for a, b, _, _, _ in lines] == [(k, j) for k in range(K) for j in range(1, steps + 1)], out
    ens = {(int(a), int(b)): (kin, pot, work) for a, b, kin, pot, work in lines}
    growth = re.findall(GROWTH_LINE, out, re.M)
    assert growth and all(gl[0] == "gauss" for gl in growth), out
    m = re.search(r"^SLOD irk wave ensemble of 3 at T = 0.02: L2 norm of the mean = (\S+), of the standard deviation = (\S+)$",
                  out, re.M)
    assert m and float(m.group(1)) > 0.0 and float(m.group(2)) > 0.0, out
    for k in range(K):
        one = _driver("--member", str(k), "--wave", str(steps), dt, "--irk", "gauss")
        rows = re.findall(r"^wave step (\d+): kinetic = (\S+), potential = (\S+), work = (\S+)$", one, re.M)
        assert [int(r[0]) for r in rows] == list(range(1, steps + 1)), one
        for j, kin, pot, work in rows:
            assert ens[(k, int(j))] == (kin, pot, work), (k, j, ens[(k, int(j))], (kin, pot, work))
        if k == 0:                                                   # the factor line of member 0
            assert re.findall(GROWTH_LINE, one, re.M)[-1] == growth[-1]
        kin, pot, work = (np.array([float(ens[(k, j)][i]) for j in range(1, steps + 1)]) for i in range(3))
        gap = np.abs(kin + pot - work).max() / pot.max()
        print("member %d: largest |kinetic + potential - work| / max potential %.3e" % (k, gap))
        assert (kin > 0).all() and (pot > 0).all() and gap <= 1e-8, (k, kin, pot, work)
    assert len({ens[(k, steps)] for k in range(K)}) == K            # the members differ


def test_driver_ensemble_irk_heat():
    """The same with --heat: the distances of member m to its elliptic solution are those of the single --member m run."""
    K, steps, dt = 3, 4, "0.01"
    out = _driver("--ensemble", str(K), "--heat", str(steps), dt, "--irk", "gauss")
    lines = re.findall(r"^member (\d+) irk heat step (\d+): L2 distance = (\S+), energy distance = (\S+)$", out, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(k, j) for j in range(1, steps + 1) for k in range(K)], out
    ens = {(int(a), int(b)): (l2, en) for a, b, l2, en in lines}
    m = re.search(r"^SLOD irk heat ensemble of 3 at T = 0.04: L2 norm of the mean = (\S+), of the standard deviation = (\S+)$",
                  out, re.M)
    assert m and float(m.group(1)) > 0.0 and float(m.group(2)) > 0.0, out
    assert re.findall(GROWTH_LINE, out, re.M), out
    for k in range(K):
        one = _driver("--member", str(k), "--heat", str(steps), dt, "--irk", "gauss")
        table = one.split("vs elliptic SLOD solution")[1]
        err = dict(re.findall(r"^  (\S+) +error = (\S+)", table, re.M))
        assert ens[(k, steps)] == (err["L2"], err["energy"]), (k, ens[(k, steps)], err)
        d = np.array([float(ens[(k, j)][0]) for j in range(1, steps + 1)])
        assert (np.diff(d) < 0.0).all(), (k, d)                       # towards the elliptic solution
    assert len({ens[(k, steps)] for k in range(K)}) == K
