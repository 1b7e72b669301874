"""CPU-side checks of the sponge-layer calls (slod_lod_newmark_accel_damped, slod_lod_newmark_steps_damped, their _direct
forms, slod_lod_factor_create_zldl3, slod_lod_irk_damping_coefficient, slod_lod_irk_wave_steps_damped_direct,
slod_lod_harmonic_response_damped), after the pattern of test_lod_irk_abi.py: the calls are exported, declared with the
signatures of include/slod.h and wrapped; the header carries the formulas and refusals; the host-only helper returns
z = dt lambda; and every SLOD_ERR_ARGUMENT that needs no device is returned before any device work with the call's name in
slod_last_error.  The refusals that need a factor are in test_gpu_lod_sponge.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lod_irk_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF, INF = float("nan"), float("inf")

SIGNATURES = {
    "slod_lod_newmark_accel_damped": "slod_handle* double* double* double* uint32_t* double double int double* size_t double* "
                                     "size_t double* size_t double* size_t double int int* double*",
    "slod_lod_newmark_steps_damped": "slod_handle* double* double* double* uint32_t* double double double double double int int "
                                     "double* size_t double* size_t double* size_t double* size_t size_t double int int* double* "
                                     "double* double*",
    "slod_lod_newmark_accel_damped_direct": "slod_handle* slod_lod_factor* double* double* double* uint32_t* double double int "
                                            "double* size_t double* size_t double* size_t double* size_t",
    "slod_lod_newmark_steps_damped_direct": "slod_handle* slod_lod_factor* double* double* double* uint32_t* double double double "
                                            "double double int int double* size_t double* size_t double* size_t double* size_t "
                                            "size_t double* double*",
    "slod_lod_factor_create_zldl3": "slod_handle* double* double* double* uint32_t* double* double* double* int int32_t* "
                                    "slod_lod_factor**",
    "slod_lod_irk_damping_coefficient": "int double double*",
    "slod_lod_irk_wave_steps_damped_direct": "slod_handle* slod_lod_factor* int int double* double* double* uint32_t* double "
                                             "double double int int double* size_t double* size_t double* size_t size_t double* "
                                             "double*",
    "slod_lod_harmonic_response_damped": "slod_handle* double* double* double* uint32_t* double double double* int double* "
                                         "double* size_t int double* double* size_t double* double* double*",
}
SCALARS = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t}


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def _header():
    return open(os.path.join(ROOT, "include", "slod.h")).read()


def _declared_types(name):
    m = re.search(r"^int %s\((.*?)\);" % name, _header(), re.M | re.S)
    assert m, "not declared: " + name
    out = []
    for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        p = p.replace("const", " ").strip()
        stars = p.count("*") + p.count("[")          # double gamma[2] is a pointer
        words = re.sub(r"\[\d*\]", " ", p).replace("*", " ").split()
        out.append(" ".join(words[:-1]) + "*" * stars)
    return out


def test_sponge_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n, sig in SIGNATURES.items():
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = sig.split()
        assert _declared_types(n) == want, (n, _declared_types(n))
        got = getattr(lib, n).argtypes
        assert len(got) == len(want), n
        for t, w in zip(got, want):
            if w.endswith("*"):
                assert t is C.c_void_p or issubclass(t, C._Pointer), (n, w, t)
            else:
                assert t is SCALARS[w], (n, w, t)
    assert lib.slod_abi_version() == 5
    for m in ("lod_factor_zldl3", "lod_irk_damping_coefficient"):
        assert callable(getattr(slod_amd.Slod, m))
    import inspect
    for m in ("lod_newmark_accel", "lod_newmark_steps", "lod_newmark_accel_direct", "lod_newmark_steps_direct", "lod_irk_wave_steps",
              "lod_harmonic_response"):
        assert inspect.signature(getattr(slod_amd.Slod, m)).parameters["d_damping"].default is None, m


def test_header_documents_the_sponge():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())
    for promised in ("M u'' + (damp_mass M + damp_stiff A + D) u' + A u = b(t)",
                     "d_damping == NULL means D = 0",
                     "M a = b^0 - A (u + damp_stiff v) - damp_mass M v - D v",
                     "S = (1 + gamma dt damp_mass) M + (beta dt^2 + gamma dt damp_stiff) A + (gamma dt) D",
                     "g = ((b - A w) - damp_mass (M v~)) - (D v~)",
                     "two slod_lod_matrix_combine roundings",
                     "S_k = alpha_k A + beta_k B + gamma_k C",
                     "re = ((alpha_re a) + (beta_re b)) + (gamma_re c)",
                     "S = (1 + z damp_mass) M + (z damp_stiff + z^2) A + z D",
                     "r = tau_1 b_1 + tau_2 b_2 - sigma [A (u + (z + damp_stiff) v) + damp_mass M v + D v]",
                     "S(omega) = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M + i omega D",
                     "(u^H M u, u^H A u, u^H D u, Re u^H b, Im u^H b)",
                     "omega (damp_mass u^H M u + damp_stiff u^H A u + u^H D u) = Im u^H b",
                     "Semi-definiteness is the caller's business",
                     "the existence of the factor is then the caller's risk and the growth is reported",
                     "Not built: ensemble forms of the four damped calls and of slod_lod_factor_create_zldl3"):
        assert promised in flat, promised
    for word in ("theta-scheme or heat calls", "the eigen calls", "perfectly matched layers", "a refresh of D after slod_update_coefficient",
                 "the deal.II adapter"):
        assert word in flat[flat.index("Not built: ensemble forms of the four damped calls"):], word


@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
def test_damping_coefficient_is_dt_lambda(label, scheme):
    slod_amd, g = _handle(nref=2)
    r3, r2 = np.sqrt(np.longdouble(3)), np.sqrt(np.longdouble(2))
    lr, li = (np.longdouble(1) / 4, r3 / 12) if scheme == ic.GAUSS else (np.longdouble(1) / 3, r2 / 6)
    for dt in (1e-3, 0.37, 5.0, 2.0 ** -20):
        z = g.lod_irk_damping_coefficient(scheme, dt)
        assert z == g.lod_irk_damping_coefficient(label, dt)
        assert z.real == float(np.longdouble(dt) * lr) and z.imag == float(np.longdouble(dt) * li), (label, dt, z)
        assert abs(z - dt * ic.LAMBDA[scheme]) <= 4e-16 * abs(z)


def test_damping_coefficient_argument_checks():
    slod_amd = _handle(nref=2)[0]
    lib = slod_amd.load()
    gam = (C.c_double * 2)()
    name = "slod_lod_irk_damping_coefficient"
    ok = [0, 0.1, gam]
    for at, bad, word in ((0, -1, "scheme"), (0, 2, "scheme"), (1, 0.0, "dt"), (1, -1.0, "dt"), (1, NANF, "dt"), (1, INF, "dt"),
                          (2, None, "NULL")):
        args = list(ok)
        args[at] = bad
        assert lib.slod_lod_irk_damping_coefficient(*args) == -1, (at, bad)
        msg = lib.slod_last_error(None).decode()
        assert msg.startswith(name + ":") and word in msg, (at, bad, msg)
    assert lib.slod_lod_irk_damping_coefficient(*ok) == 0


def _refused(g, name, ok, cases, word=None):
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        msg = g.lib.slod_last_error(g.h).decode()
        assert msg.startswith(name + ":"), (name, at, bad, msg)
        if word:
            assert word in msg, (name, at, bad, msg)


@pytest.mark.parametrize("damping", [FAKE, None])
def test_newmark_damped_argument_checks(damping):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    n, steps = 2, 3
    kin, pot = (C.c_double * ((steps + 1) * n))(), (C.c_double * ((steps + 1) * n))()
    its, res = (C.c_int * steps)(), (C.c_double * steps)()
    # (h, A, M, D, cols, dm, ds, n_rhs, u, ld_u, v, ld_v, load, ld_load, a, ld_a, rel_tol, max_it, its, res)
    name = "slod_lod_newmark_accel_damped"
    ok = [g.h, FAKE, FAKE, damping, FAKE, 0.1, 0.0, n, FAKE, n, FAKE, n, FAKE, n, FAKE, n, 1e-10, 10, its, res]
    _refused(g, name, ok, ((1, None), (2, None), (4, None), (8, None), (10, None), (14, None)), "NULL")
    _refused(g, name, ok, ((5, -0.1), (5, NANF), (6, -1.0)), "damping")
    _refused(g, name, ok, ((7, 0), (17, -1)), "n_rhs < 1")
    _refused(g, name, ok, ((9, n - 1), (11, n - 1), (13, n - 1), (15, n - 1)), "leading dimension")
    # (h, f, A, M, D, cols, dm, ds, n_rhs, u, ld_u, v, ld_v, load, ld_load, a, ld_a)
    name = "slod_lod_newmark_accel_damped_direct"
    ok = [g.h, None, FAKE, FAKE, damping, FAKE, 0.1, 0.0, n, FAKE, n, FAKE, n, FAKE, n, FAKE, n]
    _refused(g, name, ok, ((2, None), (3, None), (5, None), (9, None)), "NULL")
    _refused(g, name, ok, ((6, -0.1),), "damping")
    assert getattr(g.lib, name)(*ok) == -1 and g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    # (h, A, M, D, cols, dt, beta, gamma, dm, ds, n_steps, n_rhs, u, ld_u, v, ld_v, a, ld_a, load, ld_load, stride, tol, max_it,
    #  its, res, kin, pot)
    name = "slod_lod_newmark_steps_damped"
    ok = [g.h, FAKE, FAKE, damping, FAKE, 0.1, 0.25, 0.5, 0.1, 0.0, steps, n, FAKE, n, FAKE, n, FAKE, n, FAKE, n, 64, 1e-10, 10, its,
          res, kin, pot]
    _refused(g, name, ok, ((1, None), (2, None), (4, None), (12, None), (14, None), (16, None)), "NULL")
    _refused(g, name, ok, ((5, 0.0), (5, NANF), (6, 0.6), (6, -0.1), (7, 1.5)), "dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]")
    _refused(g, name, ok, ((8, -0.1), (9, NANF)), "damping")
    _refused(g, name, ok, ((10, 0), (11, 0), (22, -1)), "n_steps < 1, n_rhs < 1 or max_iterations < 0")
    _refused(g, name, ok, ((13, n - 1), (15, n - 1), (17, n - 1), (19, n - 1)), "leading dimension")
    _refused(g, name, ok, ((25, None), (26, None)), "kinetic and potential come together or not at all")
    # (h, f, A, M, D, cols, dt, beta, gamma, dm, ds, n_steps, n_rhs, u, ld_u, v, ld_v, a, ld_a, load, ld_load, stride, kin, pot)
    name = "slod_lod_newmark_steps_damped_direct"
    ok = [g.h, None, FAKE, FAKE, damping, FAKE, 0.1, 0.25, 0.5, 0.1, 0.0, steps, n, FAKE, n, FAKE, n, FAKE, n, FAKE, n, 64, kin, pot]
    _refused(g, name, ok, ((2, None), (3, None), (5, None), (13, None), (15, None), (17, None)), "NULL")
    _refused(g, name, ok, ((6, -1.0), (7, 0.75), (8, -0.5)), "dt <= 0")
    _refused(g, name, ok, ((11, 0), (12, -2)), "n_steps < 1 or n_rhs < 1")
    _refused(g, name, ok, ((22, None), (23, None)), "kinetic and potential come together or not at all")
    assert getattr(g.lib, name)(*ok) == -1 and g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_steps_direct(None, FAKE, FAKE, FAKE, -0.1, 1, FAKE, FAKE, FAKE, d_damping=FAKE)
    assert e.value.code == -1 and "slod_lod_newmark_steps_damped_direct:" in str(e.value)


def test_zldl3_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name = "slod_lod_factor_create_zldl3"
    one = lambda re, im: (C.c_double * 4)(re, im, re, im)   # noqa: E731
    out, bad = C.c_void_p(1), (C.c_int32 * 2)()
    # (h, a, b, c, cols, alpha, beta, gamma, n_members, bad_pivot, out)
    ok = [g.h, FAKE, FAKE, FAKE, FAKE, one(1.0, 0.1), one(-1.0, 0.2), one(0.0, 0.3), 2, bad, C.byref(out)]
    _refused(g, name, ok, ((1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (10, None)),
             "NULL handle, array, alpha, beta, gamma or out")
    _refused(g, name, ok, ((8, 0), (8, 65536)), "n_members < 1 or > 65535")
    for at in (5, 6, 7):
        _refused(g, name, ok, ((at, one(NANF, 0.0)), (at, one(0.0, INF)), (at, one(-INF, 0.0))), "a coefficient is NaN or infinite")
    out.value = 1
    assert getattr(g.lib, name)(*[None] + ok[1:]) == -1 and out.value is None      # out is cleared first


def test_irk_wave_damped_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name, n, steps = "slod_lod_irk_wave_steps_damped_direct", 2, 3
    kin, pot = (C.c_double * ((steps + 1) * n))(), (C.c_double * ((steps + 1) * n))()
    # (h, f, member, scheme, A, M, D, cols, dt, dm, ds, n_steps, n_rhs, u, ld_u, v, ld_v, load, ld_load, stride, kin, pot)
    for damping in (FAKE, None):
        ok = [g.h, None, 0, 1, FAKE, FAKE, damping, FAKE, 0.1, 0.1, 0.0, steps, n, FAKE, n, FAKE, n, FAKE, n, 0, kin, pot]
        _refused(g, name, ok, ((4, None), (5, None), (7, None), (13, None), (15, None)), "NULL")
        _refused(g, name, ok, ((3, -1), (3, 2)), "scheme")
        _refused(g, name, ok, ((8, 0.0), (8, -0.1), (8, NANF)), "dt")
        _refused(g, name, ok, ((9, -0.1), (9, NANF), (10, -1e-300), (10, NANF)), "damping")
        _refused(g, name, ok, ((11, 0), (11, -1), (12, 0), (12, -3)), "n_steps < 1 or n_rhs < 1")
        _refused(g, name, ok, ((14, n - 1), (16, n - 1), (18, n - 1)), "leading dimension below n_rhs")
        _refused(g, name, ok, ((20, None), (21, None)), "kinetic and potential come together or not at all")
        assert getattr(g.lib, name)(*ok) == -1 and g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"


def test_harmonic_damped_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name, n = "slod_lod_harmonic_response_damped", 2
    w = (C.c_double * 3)(1.0, 2.0, 3.0)
    bad_w = lambda x: (C.c_double * 3)(1.0, x, 3.0)   # noqa: E731
    res, growth, q = (C.c_double * 6)(), (C.c_double * 3)(), (C.c_double * 30)()
    # (h, A, M, D, cols, dm, ds, omega, n_freq, b_re, b_im, ld_load, n_rhs, u_re, u_im, ld_u, res, growth, quantities)
    for damping in (FAKE, None):
        ok = [g.h, FAKE, FAKE, damping, FAKE, 0.1, 0.0, w, 3, FAKE, FAKE, n, n, FAKE, FAKE, 3 * n, res, growth, q]
        _refused(g, name, ok, ((1, None), (2, None), (4, None), (7, None), (9, None), (13, None), (14, None)),
                 "NULL handle, matrix, d_cols, omega, load or u")
        _refused(g, name, ok, ((5, -0.1), (5, NANF), (6, INF)), "negative, NaN or infinite damping coefficient")
        _refused(g, name, ok, ((8, 0), (12, 0)), "n_freq < 1 or n_rhs < 1")
        _refused(g, name, ok, ((7, bad_w(-1.0)), (7, bad_w(NANF)), (7, bad_w(INF))), "a frequency is negative, NaN or infinite")
        _refused(g, name, ok, ((7, bad_w(1e200)),), "overflows")
        _refused(g, name, ok, ((11, n - 1),), "leading dimension of the load below n_rhs")
        _refused(g, name, ok, ((15, 3 * n - 1),), "leading dimension of u below n_freq * n_rhs")


def test_sponge_profile():
    import slod_amd
    NE, width, smax = 16, 0.25, 3.0
    sig = slod_amd.sponge_profile(NE, width, smax)
    assert sig.shape == (NE * NE,) and sig.dtype == np.float64
    for ey, ex in ((0, 0), (0, 7), (3, 9), (5, 1), (8, 8), (15, 2)):
        d = min((ex + 0.5) / NE, 1.0 - (ex + 0.5) / NE, (ey + 0.5) / NE, 1.0 - (ey + 0.5) / NE)
        assert sig[ey * NE + ex] == pytest.approx(smax * max(0.0, 1.0 - d / width) ** 2, rel=1e-14, abs=0.0), (ey, ex)
    assert (sig >= 0.0).all() and sig.max() < smax and sig[8 * NE + 8] == 0.0
    for bad in ((0, 0.25, 1.0), (4, 0.0, 1.0), (4, 0.25, -1.0)):
        with pytest.raises(ValueError):
            slod_amd.sponge_profile(*bad)


def test_sponge_without_gpu_fails_loudly():
    """No CPU fallback: the three-term factor is SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_zldl3(FAKE, FAKE, FAKE, FAKE, [1.0 + 0.1j], [1.0], [0.1j])
    assert e.value.code == -3 and "no CPU fallback" in str(e.value)
