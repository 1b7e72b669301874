"""CPU-side checks of the implicit Runge-Kutta steppers of a coefficient ensemble
(slod_lod_irk_heat_steps_ensemble_direct, slod_lod_irk_wave_steps_ensemble_direct), in the manner of test_lod_irk_abi.py:
the calls are exported by the release library, declared with the signatures of include/slod.h and wrapped in slod_amd;
and every SLOD_ERR_ARGUMENT that needs no factor is returned before any device work (so on a machine without a GPU) with
the call's name in slod_last_error.  The refusals that need a factor are in test_gpu_lod_irk_ensemble.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF, INF = float("nan"), float("inf")

SIGNATURES = {
    "slod_lod_irk_heat_steps_ensemble_direct": "slod_handle* slod_lod_factor* int int double* size_t uint32_t* double int int "
                                               "double* size_t double* size_t size_t",
    "slod_lod_irk_wave_steps_ensemble_direct": "slod_handle* slod_lod_factor* int int double* size_t double* size_t uint32_t* "
                                               "double double double int int double* size_t double* size_t double* size_t "
                                               "size_t double* double*",
}
NAMES = {
    "slod_lod_irk_heat_steps_ensemble_direct": "h f_S first_member scheme d_stiffness ld_a_m d_cols dt n_steps n_members d_u ld_u "
                                               "d_load ld_load load_stage_stride",
    "slod_lod_irk_wave_steps_ensemble_direct": "h f_S first_member scheme d_stiffness ld_a_m d_mass ld_m_m d_cols dt damp_mass "
                                               "damp_stiff n_steps n_members d_u ld_u d_v ld_v d_load ld_load load_stage_stride "
                                               "kinetic potential",
}
SCALARS = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t}


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def _header():
    return open(os.path.join(ROOT, "include", "slod.h")).read()


def _declared(name):
    """([type], [parameter name]) of the declaration in the header."""
    m = re.search(r"^int %s\((.*?)\);" % name, _header(), re.M | re.S)
    assert m, "not declared: " + name
    types, names = [], []
    for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        p = p.replace("const", " ").strip()
        stars = p.count("*")
        words = p.replace("*", " ").split()
        types.append(" ".join(words[:-1]) + "*" * stars)
        names.append(words[-1])
    return types, names


def test_ensemble_irk_symbols_are_declared_exported_and_bound():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n, sig in SIGNATURES.items():
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = sig.split()
        types, names = _declared(n)
        assert types == want, (n, types)
        assert names == NAMES[n].split(), (n, names)
        got = getattr(lib, n).argtypes
        assert got is not None and len(got) == len(want), n
        for t, w in zip(got, want):
            if w.endswith("*"):
                assert t is C.c_void_p or issubclass(t, C._Pointer), (n, w, t)
            else:
                assert t is SCALARS[w], (n, w, t)
    assert lib.slod_abi_version() == 5
    for m in ("lod_irk_heat_steps_ensemble", "lod_irk_wave_steps_ensemble"):
        assert callable(getattr(slod_amd.Slod, m))


def test_symbols_are_in_the_dynamic_table_of_the_release_library():
    import slod_amd
    path = slod_amd.load()._name
    data = open(path, "rb").read()
    for n in SIGNATURES:
        assert n.encode() + b"\0" in data, n


def test_header_documents_the_ensemble_steppers():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())
    for promised in ("factor member first_member + m",
                     "first_member = k K picks dt_k",
                     "d_load[(2 k + i) load_stage_stride + r ld_load + m]",
                     "A step is three launches, five with the energies, for any number of members",
                     "they do not depend on K, a leading dimension, the member's position, first_member or the run",
                     "members outside the factor",
                     "Not built: several columns per member, three-stage schemes, CG or PCG as the stage solver, members spread "
                     "over ranks"):
        assert promised in flat, promised
    # the f20 block no longer lists the ensemble forms as missing
    assert "ensemble forms, CG or PCG" not in flat


def _refused(g, name, ok, cases, word):
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        msg = g.lib.slod_last_error(g.h if at != 0 else None).decode()
        assert msg.startswith(name + ":") and word in msg, (name, at, bad, msg)


def test_heat_ensemble_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name, K = "slod_lod_irk_heat_steps_ensemble_direct", 3
    # (h, f, first_member, scheme, A, ld_a_m, cols, dt, n_steps, n_members, u, ld_u, load, ld_load, stride)
    ok = [g.h, None, 0, 0, FAKE, K, FAKE, 0.1, 2, K, FAKE, K, FAKE, K, 64]
    _refused(g, name, ok, ((0, None), (4, None), (6, None), (10, None)), "NULL")
    _refused(g, name, ok, ((3, -1), (3, 2)), "scheme")
    _refused(g, name, ok, ((7, 0.0), (7, -0.1), (7, NANF), (7, INF)), "dt")
    _refused(g, name, ok, ((8, 0), (8, -1), (9, 0), (9, -3)), "n_steps < 1 or n_members < 1")
    _refused(g, name, ok, ((5, K - 1), (11, K - 1), (13, K - 1)), "leading dimension below n_members")
    # everything else in order: the factor is looked at last
    assert g.lib.slod_lod_irk_heat_steps_ensemble_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    ok[12], ok[13] = None, 0                                            # no load: its leading dimension is not read
    assert g.lib.slod_lod_irk_heat_steps_ensemble_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_irk_heat_steps_ensemble(None, "radau", FAKE, FAKE, -1.0, 1, K, FAKE)
    assert e.value.code == -1 and "dt" in str(e.value)


def test_wave_ensemble_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name, K, steps = "slod_lod_irk_wave_steps_ensemble_direct", 2, 3
    kin, pot = (C.c_double * ((steps + 1) * K))(), (C.c_double * ((steps + 1) * K))()
    # (h, f, first_member, scheme, A, ld_a_m, M, ld_m_m, cols, dt, dm, ds, n_steps, n_members, u, ld_u, v, ld_v, load,
    #  ld_load, stride, kin, pot)
    ok = [g.h, None, 0, 1, FAKE, K, FAKE, K, FAKE, 0.1, 0.1, 0.0, steps, K, FAKE, K, FAKE, K, FAKE, K, 0, kin, pot]
    _refused(g, name, ok, ((0, None), (4, None), (6, None), (8, None), (14, None), (16, None)), "NULL")
    _refused(g, name, ok, ((3, -1), (3, 2)), "scheme")
    _refused(g, name, ok, ((9, 0.0), (9, -0.1), (9, NANF)), "dt")
    _refused(g, name, ok, ((10, -0.1), (10, NANF), (10, INF), (11, -1e-300), (11, NANF)), "damping")
    _refused(g, name, ok, ((12, 0), (12, -1), (13, 0), (13, -3)), "n_steps < 1 or n_members < 1")
    _refused(g, name, ok, ((5, K - 1), (7, K - 1), (15, K - 1), (17, K - 1), (19, K - 1)), "leading dimension below n_members")
    _refused(g, name, ok, ((21, None), (22, None)), "kinetic and potential come together or not at all")
    assert g.lib.slod_lod_irk_wave_steps_ensemble_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    ok[21] = ok[22] = None
    assert g.lib.slod_lod_irk_wave_steps_ensemble_direct(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_irk_wave_steps_ensemble(None, "gauss", FAKE, FAKE, FAKE, 0.1, 1, K, FAKE, FAKE, damp_stiff=-1.0)
    assert e.value.code == -1 and "damping" in str(e.value)
