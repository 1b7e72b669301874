"""CPU-side checks of the frequency response (slod_lod_factor_create_zldl, slod_lod_factor_solve_complex,
slod_lod_harmonic_response), after the pattern of test_lod_ldl_abi.py: the calls are exported, declared with the
signatures of include/slod.h and wrapped, the header documents what it promises, and every SLOD_ERR_ARGUMENT that needs
no factor is returned before any device work (so on a machine without a GPU) with the call's name in slod_last_error.
The refusals that need a factor (a real factor, members outside it, the leading dimensions and the in-place case of
slod_lod_factor_solve_complex; a complex factor given to the other consumers) are in test_gpu_lod_harmonic.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF, INF = float("nan"), float("inf")

SIGNATURES = {
    "slod_lod_factor_create_zldl": "slod_handle* double* double* uint32_t* double* double* int int32_t* slod_lod_factor**",
    "slod_lod_factor_solve_complex": "slod_lod_factor* int int double* double* size_t int int double* double* size_t void*",
    "slod_lod_harmonic_response": "slod_handle* double* double* uint32_t* double double double* int double* double* size_t int "
                                  "double* double* size_t double* double*",
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


def test_harmonic_symbols_are_exported_and_declared():
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
    for m in ("lod_factor_zldl", "lod_harmonic_response"):
        assert callable(getattr(slod_amd.Slod, m))
    for m in ("solve_complex", "inertia", "member_info", "close"):
        assert callable(getattr(slod_amd.ComplexFactor, m))
    assert issubclass(slod_amd.ComplexFactor, slod_amd.Factor)


def test_header_documents_the_frequency_response():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())           # without the comment's left margin
    for promised in ("S(omega) = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M",
                     "complex SYMMETRIC (not Hermitian)",
                     "re = (alpha_re a) + (beta_re b), im = (alpha_im a) + (beta_im b)",
                     "ONLY THE LOWER TRIANGLE IN FACTOR ORDER IS READ",
                     "n_negative = n_positive = -1",
                     "member k: pivot r of n is zero or not finite (re, im)",
                     "frequency k: pivot r of n is zero or not finite (re, im)",
                     "a complex factor (slod_lod_factor_create_zldl) is solved by slod_lod_factor_solve_complex",
                     "chunks of at most 64 frequencies",
                     "Not built: coefficient ensembles x frequencies, 2 x 2 pivots, damping that is not Rayleigh, adaptive "
                     "frequency refinement, this factor as a preconditioner"):
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


def test_create_zldl_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    K = 3
    out = C.c_void_p(1)
    bad = (C.c_int32 * K)()
    keep_a, alpha = _pairs(1.0, 1.0 + 0.5j, 2.0)
    keep_b, beta = _pairs(-1.0, -2.0 + 0.1j, 0.3j)
    name = "slod_lod_factor_create_zldl"
    ok = [g.h, FAKE, FAKE, FAKE, alpha, beta, K, bad, C.byref(out)]
    _refused(g, name, ok, ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (8, None)), "NULL")
    assert out.value is None                                             # *out is cleared before the checks
    _refused(g, name, ok, ((6, 0), (6, -1), (6, 65536)), "n_members")
    for which in (4, 5):
        for at in range(2 * K):
            for v in (NANF, INF, -INF):
                keep, ptr = _pairs(1.0, 1.0 + 0.5j, 2.0)
                keep[at] = v
                _refused(g, name, ok, ((which, ptr),), "NaN or infinite")
    # through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_zldl(None, FAKE, FAKE, [1.0], [1j])
    assert e.value.code == -1 and name + ":" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_zldl(FAKE, FAKE, FAKE, [1.0, complex(NANF, 0.0)], [1j, 2j])
    assert e.value.code == -1 and "NaN or infinite" in str(e.value) and (e.value.bad_pivot == -1).all()
    with pytest.raises(ValueError):
        g.lod_factor_zldl(FAKE, FAKE, FAKE, [1.0, 2.0], [1j])


def test_solve_complex_refuses_a_null_factor():
    slod_amd = _handle(nref=2)[0]
    lib = slod_amd.load()
    assert lib.slod_lod_factor_solve_complex(None, 0, 1, FAKE, FAKE, 1, 1, 0, FAKE, FAKE, 1, None) == -1
    assert "slod_lod_factor_solve_complex: NULL factor" in lib.slod_last_error(None).decode()


def test_harmonic_response_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    nf, n = 3, 2
    w = (C.c_double * nf)(1.0, 2.0, 0.0)
    res, growth = (C.c_double * (nf * n))(), (C.c_double * nf)()
    name = "slod_lod_harmonic_response"
    # (h, A, M, cols, damp_mass, damp_stiff, omega, n_freq, load_re, load_im, ld_load, n_rhs, u_re, u_im, ld_u, res, growth)
    ok = [g.h, FAKE, FAKE, FAKE, 0.1, 0.0, w, nf, FAKE, None, n, n, FAKE, FAKE, nf * n, res, growth]
    _refused(g, name, ok, ((0, None), (1, None), (2, None), (3, None), (6, None), (8, None), (12, None), (13, None)), "NULL")
    _refused(g, name, ok, ((4, -0.1), (4, NANF), (4, INF), (5, -1e-300), (5, NANF), (5, INF)), "damping")
    _refused(g, name, ok, ((7, 0), (7, -1), (11, 0), (11, -2)), "n_freq < 1 or n_rhs < 1")
    for v in (-1.0, NANF, INF, -INF):
        for at in range(nf):
            bad = (C.c_double * nf)(1.0, 2.0, 0.0)
            bad[at] = v
            _refused(g, name, ok, ((6, bad),), "frequency")
    _refused(g, name, ok, ((6, (C.c_double * nf)(1.0, 1e200, 0.0)),), "overflows")
    _refused(g, name, ok, ((10, n - 1),), "leading dimension of the load")
    _refused(g, name, ok, ((14, nf * n - 1), (14, n)), "leading dimension of u below n_freq * n_rhs")
    # through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_harmonic_response(FAKE, FAKE, FAKE, [1.0, -2.0], FAKE, None, FAKE, FAKE)
    assert e.value.code == -1 and "frequency" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_harmonic_response(FAKE, FAKE, FAKE, [1.0, 2.0], FAKE, None, FAKE, FAKE, n_rhs=2, ld_u=3)
    assert e.value.code == -1 and "n_freq * n_rhs" in str(e.value)
