"""CPU-side checks of the ensemble frequency response (slod_lod_factor_create_zldl_ensemble,
slod_lod_factor_solve_complex_ensemble, slod_lod_harmonic_response_ensemble), after the pattern of
test_lod_harmonic_abi.py: the calls are exported, declared with the signatures of include/slod.h and wrapped, the header
documents the layout, the messages and what is not built, and every SLOD_ERR_ARGUMENT that needs no factor is returned
before any device work (so on a machine without a GPU) with the call's name in slod_last_error.  The refusals that need a
factor are in test_gpu_lod_harmonic_ensemble.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF, INF = float("nan"), float("inf")

SIGNATURES = {
    "slod_lod_factor_create_zldl_ensemble": "slod_handle* double* size_t double* size_t int uint32_t* double* double* int int32_t* "
                                            "slod_lod_factor**",
    "slod_lod_factor_solve_complex_ensemble": "slod_lod_factor* int int double* double* size_t int int double* double* size_t void*",
    "slod_lod_harmonic_response_ensemble": "slod_handle* double* size_t double* size_t uint32_t* int double double double* int double* "
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
        words = p.replace("*", " ").split()
        out.append(" ".join(words[:-1]) + "*" * p.count("*"))
    return out


def test_ensemble_harmonic_symbols_are_exported_and_declared():
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
    for m in ("lod_factor_zldl_ensemble", "lod_harmonic_response_ensemble"):
        assert callable(getattr(slod_amd.Slod, m))
    import inspect
    assert "rhs_members" in inspect.signature(slod_amd.ComplexFactor.solve_complex).parameters


def test_header_documents_the_ensemble_frequency_response():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())           # without the comment's left margin
    for promised in ("factor member j = k K + m is S_j = alpha_k A_m + beta_k B_m",
                     "column (k K + m) n_rhs + c of (d_u_re, d_u_im)",
                     "Member m's loads are the columns m n_rhs + c of d_load",
                     "slod_lod_reconstruct_ensemble, slod_lod_inner_ensemble and slod_ensemble_moments apply to a frequency's block",
                     "by pointer offset with ld = F K",
                     "chunks of at most 64 consecutive j",
                     "quantities[col] = (u^H M u, u^H A u, Re u^H b, Im u^H b)",
                     "A zero load column gives four exact zeros",
                     "omega (damp_mass u^H M u + damp_stiff u^H A u) = Im u^H b",
                     "slod_lod_harmonic_response_ensemble: frequency k, member m: pivot r of n is zero or not finite (re, im)",
                     "\"coefficient k, member m\"",
                     "never read or written",
                     "Not built: members or frequencies spread over ranks, 2 x 2 pivots, damping that is not Rayleigh, adaptive "
                     "frequency refinement, the complex factor as a preconditioner, output functionals other than u^H b"):
        assert promised in flat, promised


def _refused(g, name, ok, cases, word=None):
    """Every (position, bad value) alone makes the call return SLOD_ERR_ARGUMENT and leaves the call's name in the
    handle's error text (a NULL handle leaves it in the thread's)."""
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        if at != 0:
            msg = g.lib.slod_last_error(g.h).decode()
            assert msg.startswith(name + ":"), (name, at, bad, msg)
            if word:
                assert word in msg, (name, at, bad, msg)


def _pairs(*zs):
    a = np.array(zs, dtype=np.complex128).view(np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def test_create_zldl_ensemble_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    K, F = 3, 2
    out = C.c_void_p(1)
    bad = (C.c_int32 * (K * F))()
    keep_a, alpha = _pairs(1.0, 1.0 + 0.5j)
    keep_b, beta = _pairs(-1.0, -2.0 + 0.1j)
    name = "slod_lod_factor_create_zldl_ensemble"
    # (h, a, ld_a_m, b, ld_b_m, n_members, cols, alpha, beta, n_coef, bad_pivot, out)
    ok = [g.h, FAKE, K + 1, FAKE, K, K, FAKE, alpha, beta, F, bad, C.byref(out)]
    _refused(g, name, ok, ((0, None), (1, None), (3, None), (6, None), (7, None), (8, None), (11, None)), "NULL")
    assert out.value is None                                             # *out is cleared before the checks
    _refused(g, name, ok, ((5, 0), (5, -1), (5, 65536)), "n_members < 1 or > 65535")
    _refused(g, name, ok, ((9, 0), (9, -1), (9, 65535 // K + 1)), "n_coef")
    _refused(g, name, ok, ((2, K - 1), (4, K - 1), (2, 0)), "leading dimension of a matrix below n_members")
    for which in (7, 8):
        for at in range(2 * F):
            for v in (NANF, INF, -INF):
                keep, ptr = _pairs(1.0, 1.0 + 0.5j)
                keep[at] = v
                _refused(g, name, ok, ((which, ptr),), "NaN or infinite")
    # through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_zldl_ensemble(FAKE, FAKE, FAKE, 3, [1.0], [1j], ld_a_m=2)
    assert e.value.code == -1 and name + ":" in str(e.value) and (e.value.bad_pivot == -1).all()
    with pytest.raises(ValueError):
        g.lod_factor_zldl_ensemble(FAKE, FAKE, FAKE, 3, [1.0, 2.0], [1j])


def test_solve_complex_ensemble_refuses_a_null_factor():
    slod_amd = _handle(nref=2)[0]
    lib = slod_amd.load()
    assert lib.slod_lod_factor_solve_complex_ensemble(None, 0, 1, FAKE, FAKE, 1, 1, 1, FAKE, FAKE, 1, None) == -1
    assert "slod_lod_factor_solve_complex_ensemble: NULL factor" in lib.slod_last_error(None).decode()


def test_harmonic_response_ensemble_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    nf, n, K = 3, 2, 4
    w = (C.c_double * nf)(1.0, 2.0, 0.0)
    res, growth, q = (C.c_double * (nf * K * n))(), (C.c_double * (nf * K))(), (C.c_double * (nf * K * n * 4))()
    name = "slod_lod_harmonic_response_ensemble"
    # (h, A, ld_a_m, M, ld_m_m, cols, K, damp_mass, damp_stiff, omega, n_freq, load_re, load_im, ld_load, n_rhs, u_re, u_im,
    #  ld_u, res, growth, quantities)
    ok = [g.h, FAKE, K, FAKE, K + 2, FAKE, K, 0.1, 0.0, w, nf, FAKE, None, K * n, n, FAKE, FAKE, nf * K * n, res, growth, q]
    _refused(g, name, ok, ((0, None), (1, None), (3, None), (5, None), (9, None), (11, None), (15, None), (16, None)), "NULL")
    _refused(g, name, ok, ((6, 0), (6, -3), (6, 65536)), "n_members < 1 or > 65535")
    _refused(g, name, ok, ((7, -0.1), (7, NANF), (7, INF), (8, -1e-300), (8, NANF), (8, INF)), "damping")
    _refused(g, name, ok, ((10, 0), (10, -1), (14, 0), (14, -2)), "n_freq < 1 or n_rhs < 1")
    for v in (-1.0, NANF, INF, -INF):
        for at in range(nf):
            bad = (C.c_double * nf)(1.0, 2.0, 0.0)
            bad[at] = v
            _refused(g, name, ok, ((9, bad),), "frequency")
    _refused(g, name, ok, ((9, (C.c_double * nf)(1.0, 1e200, 0.0)),), "overflows")
    _refused(g, name, ok, ((2, K - 1), (4, K - 1), (4, 0)), "leading dimension of a matrix below n_members")
    _refused(g, name, ok, ((13, K * n - 1), (13, n)), "leading dimension of the load below n_members * n_rhs")
    _refused(g, name, ok, ((17, nf * K * n - 1), (17, K * n)), "leading dimension of u below n_freq * n_members * n_rhs")
    # through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_harmonic_response_ensemble(FAKE, FAKE, FAKE, 2, [1.0, -2.0], FAKE, None, FAKE, FAKE)
    assert e.value.code == -1 and name + ":" in str(e.value) and "frequency" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_harmonic_response_ensemble(FAKE, FAKE, FAKE, 2, [1.0, 2.0], FAKE, None, FAKE, FAKE, n_rhs=2, ld_u=7)
    assert e.value.code == -1 and "n_freq * n_members * n_rhs" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_harmonic_response_ensemble(FAKE, FAKE, FAKE, 0, [1.0], FAKE, None, FAKE, FAKE)
    assert e.value.code == -1 and "n_members" in str(e.value)
