"""CPU-side checks of the two-stage implicit Runge-Kutta steppers (slod_lod_irk_coefficients,
slod_lod_irk_heat_steps_direct, slod_lod_irk_wave_steps_direct), after the pattern of test_lod_harmonic_abi.py: the calls
are exported, declared with the signatures of include/slod.h and wrapped; the coefficient helper, which is host only,
returns the closed-form pair; and every SLOD_ERR_ARGUMENT that needs no factor is returned before any device work (so on a
machine without a GPU) with the call's name in slod_last_error.  A factor cannot exist without a device, so the refusals
that need one (a real factor, a member outside it, another handle) are in test_gpu_lod_irk.py, and SLOD_ERR_DEVICE without
a GPU is met where the steppers' factor would be built: slod_lod_factor_create_zldl on the helper's pair."""
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
    "slod_lod_irk_coefficients": "int int double double double double* double*",
    "slod_lod_irk_heat_steps_direct": "slod_handle* slod_lod_factor* int int double* uint32_t* double int int double* size_t "
                                      "double* size_t size_t",
    "slod_lod_irk_wave_steps_direct": "slod_handle* slod_lod_factor* int int double* double* uint32_t* double double double "
                                      "int int double* size_t double* size_t double* size_t size_t double* double*",
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
        stars = p.count("*") + p.count("[")          # double alpha[2] is a pointer
        words = re.sub(r"\[\d*\]", " ", p).replace("*", " ").split()
        out.append(" ".join(words[:-1]) + "*" * stars)
    return out


def test_irk_symbols_are_exported_and_declared():
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
    for m in ("lod_irk_coefficients", "lod_irk_heat_steps", "lod_irk_wave_steps"):
        assert callable(getattr(slod_amd.Slod, m))
    assert (slod_amd.IRK_GAUSS2, slod_amd.IRK_RADAU2A) == (0, 1)
    assert re.search(r"SLOD_IRK_GAUSS2\s*=\s*0\s*,\s*SLOD_IRK_RADAU2A\s*=\s*1", _header())


def test_header_documents_the_steppers():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())
    for promised in ("lambda = 1/4 + i sqrt(3)/12", "lambda = 1/3 + i sqrt(2)/6",
                     "S = (1 + z damp_mass) M + (z damp_stiff + z^2) A",
                     "stage i (0, 1) of step k is at d_load + (2 k + i) load_stage_stride",
                     "takes a complex factor (slod_lod_factor_create_zldl)",
                     "one call with n_steps = 2 equals two calls with n_steps = 1",
                     "Not built: three-stage schemes"):
        assert promised in flat, promised


def _close(got, want):
    return abs(got - want) <= 1e-15 * abs(want) if want != 0.0 else got == 0.0


@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
def test_coefficients_equal_the_closed_form(label, scheme):
    slod_amd, g = _handle(nref=2)
    r3, r2 = np.sqrt(np.longdouble(3)), np.sqrt(np.longdouble(2))
    # the parts of lambda in extended precision
    lr, li = (np.longdouble(1) / 4, r3 / 12) if scheme == ic.GAUSS else (np.longdouble(1) / 3, r2 / 6)
    for dt in (1e-3, 0.37, 5.0, 2.0 ** -20):
        dtl = np.longdouble(dt)
        zr, zi = dtl * lr, dtl * li
        a, b = g.lod_irk_coefficients(scheme, 1, dt)
        assert _close(a.real, float(zr)) and _close(a.imag, float(zi)) and b == 1.0
        assert (a, b) == g.lod_irk_coefficients(label, 1, dt)
        for dm, ds in ((0.0, 0.0), (0.3, 0.0), (0.0, 2e-3), (0.3, 2e-3)):
            a, b = g.lod_irk_coefficients(scheme, 2, dt, dm, ds)
            dml, dsl = np.longdouble(dm), np.longdouble(ds)
            want_a = (zr * dsl + (zr * zr - zi * zi), zi * dsl + 2 * zr * zi)
            want_b = (1 + zr * dml, zi * dml)
            for got, want in ((a.real, want_a[0]), (a.imag, want_a[1]), (b.real, want_b[0]), (b.imag, want_b[1])):
                assert _close(got, float(want)), (label, dt, dm, ds, got, float(want))
            # and the module's complex128 version of the same pair, the one the yardstick is built from
            ya, yb = ic.coefficients(scheme, 2, dt, dm, ds)
            assert abs(a - ya) <= 4e-16 * abs(ya) and abs(b - yb) <= 4e-16 * abs(yb)


def test_coefficients_argument_checks():
    slod_amd = _handle(nref=2)[0]
    lib = slod_amd.load()
    a, b = (C.c_double * 2)(), (C.c_double * 2)()
    name = "slod_lod_irk_coefficients"
    ok = [0, 2, 0.1, 0.0, 0.0, a, b]
    cases = ((0, -1, "scheme"), (0, 2, "scheme"), (1, 0, "order"), (1, 3, "order"), (2, 0.0, "dt"), (2, -1.0, "dt"),
             (2, NANF, "dt"), (2, INF, "dt"), (3, -0.1, "damping"), (3, NANF, "damping"), (4, -1e-300, "damping"),
             (4, NANF, "damping"), (5, None, "NULL"), (6, None, "NULL"), (2, 1e200, "overflows"))
    for at, bad, word in cases:
        args = list(ok)
        args[at] = bad
        assert lib.slod_lod_irk_coefficients(*args) == -1, (at, bad)
        msg = lib.slod_last_error(None).decode()
        assert msg.startswith(name + ":") and word in msg, (at, bad, msg)
    for dm, ds in ((0.1, 0.0), (0.0, 0.1)):
        assert lib.slod_lod_irk_coefficients(0, 1, 0.1, dm, ds, a, b) == -1
        assert "order 1" in lib.slod_last_error(None).decode()
    assert lib.slod_lod_irk_coefficients(*ok) == 0
    g = slod_amd.Slod(nref=2)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_irk_coefficients("gauss", 1, -1.0)
    assert e.value.code == -1 and name + ":" in str(e.value)


def _refused(g, name, ok, cases, word=None):
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        msg = g.lib.slod_last_error(g.h if at != 0 else None).decode()
        assert msg.startswith(name + ":"), (name, at, bad, msg)
        if word:
            assert word in msg, (name, at, bad, msg)


def test_heat_steps_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name, n = "slod_lod_irk_heat_steps_direct", 3
    # (h, f, member, scheme, A, cols, dt, n_steps, n_rhs, u, ld_u, load, ld_load, stride)
    ok = [g.h, None, 0, 0, FAKE, FAKE, 0.1, 2, n, FAKE, n, FAKE, n, 64]
    _refused(g, name, ok, ((0, None), (4, None), (5, None), (9, None)), "NULL")
    _refused(g, name, ok, ((3, -1), (3, 2)), "scheme")
    _refused(g, name, ok, ((6, 0.0), (6, -0.1), (6, NANF)), "dt")
    _refused(g, name, ok, ((7, 0), (7, -1), (8, 0), (8, -3)), "n_steps < 1 or n_rhs < 1")
    _refused(g, name, ok, ((10, n - 1), (12, n - 1)), "leading dimension below n_rhs")
    # everything else in order: the factor is looked at last
    assert g.lib.slod_lod_irk_heat_steps_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    ok[11], ok[12] = None, 0                                            # no load: its leading dimension is not read
    assert g.lib.slod_lod_irk_heat_steps_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_irk_heat_steps(None, "radau", FAKE, FAKE, -1.0, 1, FAKE)
    assert e.value.code == -1 and "dt" in str(e.value)


def test_wave_steps_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name, n, steps = "slod_lod_irk_wave_steps_direct", 2, 3
    kin, pot = (C.c_double * ((steps + 1) * n))(), (C.c_double * ((steps + 1) * n))()
    # (h, f, member, scheme, A, M, cols, dt, dm, ds, n_steps, n_rhs, u, ld_u, v, ld_v, load, ld_load, stride, kin, pot)
    ok = [g.h, None, 0, 1, FAKE, FAKE, FAKE, 0.1, 0.1, 0.0, steps, n, FAKE, n, FAKE, n, FAKE, n, 0, kin, pot]
    _refused(g, name, ok, ((0, None), (4, None), (5, None), (6, None), (12, None), (14, None)), "NULL")
    _refused(g, name, ok, ((3, -1), (3, 2)), "scheme")
    _refused(g, name, ok, ((7, 0.0), (7, -0.1), (7, NANF)), "dt")
    _refused(g, name, ok, ((8, -0.1), (8, NANF), (9, -1e-300), (9, NANF)), "damping")
    _refused(g, name, ok, ((10, 0), (10, -1), (11, 0), (11, -3)), "n_steps < 1 or n_rhs < 1")
    _refused(g, name, ok, ((13, n - 1), (15, n - 1), (17, n - 1)), "leading dimension below n_rhs")
    _refused(g, name, ok, ((19, None), (20, None)), "kinetic and potential come together or not at all")
    assert g.lib.slod_lod_irk_wave_steps_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    ok[19] = ok[20] = None
    assert g.lib.slod_lod_irk_wave_steps_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_irk_wave_steps(None, "gauss", FAKE, FAKE, FAKE, 0.1, 1, FAKE, FAKE, damp_stiff=-1.0)
    assert e.value.code == -1 and "damping" in str(e.value)


def test_irk_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly.  The coefficient helper is host only and answers; the
    factor of its pair is SLOD_ERR_DEVICE without a HIP device, and without a factor the steppers have nothing to run
    on: they refuse the NULL factor."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    alpha, beta = g.lod_irk_coefficients("gauss", 2, 0.01, 0.1, 1e-3)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_zldl(FAKE, FAKE, FAKE, [alpha], [beta])
    assert e.value.code == -3 and "no CPU fallback" in str(e.value)
    for call in (lambda: g.lod_irk_heat_steps(None, "radau", FAKE, FAKE, 0.01, 2, FAKE, n_rhs=2),
                 lambda: g.lod_irk_wave_steps(None, "gauss", FAKE, FAKE, FAKE, 0.01, 2, FAKE, FAKE, n_rhs=2)):
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and "NULL factor" in str(e.value)
