"""CPU-side checks of Newmark time stepping on a coefficient ensemble (slod_lod_inner_ensemble,
slod_lod_newmark_accel_ensemble_direct, slod_lod_newmark_steps_ensemble_direct): the calls are exported, declared with
the signatures of include/slod.h and wrapped, and every SLOD_ERR_ARGUMENT that needs no factor is returned before any
device work (so it is returned on a machine without a GPU) with the call's name in slod_last_error.  The refusals that
need a factor (another member count, the single stepper on a factor of several members) are in
test_gpu_lod_ensemble_wave.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slod_lod_inner_ensemble", "slod_lod_newmark_accel_ensemble_direct", "slod_lod_newmark_steps_ensemble_direct")
WRAPPERS = ("lod_inner_ensemble", "lod_newmark_accel_ensemble_direct", "lod_newmark_steps_ensemble_direct")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF = float("nan")

# the parameter types of include/slod.h, in order
SIGNATURES = {
    "slod_lod_inner_ensemble": "slod_handle* double* size_t uint32_t* double* size_t double* size_t int double* void*",
    "slod_lod_newmark_accel_ensemble_direct": "slod_handle* slod_lod_factor* double* size_t double* size_t uint32_t* double double "
                                              "int double* size_t double* size_t double* size_t double* size_t",
    "slod_lod_newmark_steps_ensemble_direct": "slod_handle* slod_lod_factor* double* size_t double* size_t uint32_t* double double "
                                              "double double double int int double* size_t double* size_t double* size_t double* "
                                              "size_t size_t double* double*",
}
CTYPES = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t, "double*": (C.c_void_p, C.POINTER(C.c_double))}


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def _declared_types(name):
    """The parameter types of `name` as include/slod.h declares them: comments and names dropped, const dropped."""
    text = open(os.path.join(ROOT, "include", "slod.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S)
    assert m, "not declared: " + name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    out = []
    for p in params:
        p = p.replace("const", " ").strip()
        stars = p.count("*")
        words = p.replace("*", " ").split()
        out.append(" ".join(words[:-1]) + "*" * stars)
    return out


def test_lod_ensemble_wave_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = SIGNATURES[n].split()
        assert _declared_types(n) == want, (n, _declared_types(n))
        # the binding passes what the header declares
        got = getattr(lib, n).argtypes
        assert len(got) == len(want), n
        for t, w in zip(got, want):
            if w.endswith("*"):
                assert t in CTYPES.get(w, (C.c_void_p,)), (n, w, t)
            else:
                assert t is CTYPES[w], (n, w, t)
    assert lib.slod_abi_version() == 5
    for m in WRAPPERS:
        assert callable(getattr(slod_amd.Slod, m))


def _refused(g, name, ok, cases):
    """Every (position, bad value) alone makes the call return SLOD_ERR_ARGUMENT and leaves the call's name in the
    handle's error text (a NULL handle leaves it in the thread's)."""
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        assert name in g.lib.slod_last_error(None if at == 0 else g.h).decode(), (name, at, bad)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_ensemble_wave_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    K = 3
    out = (C.c_double * K)()
    kin, pot = (C.c_double * (2 * K))(), (C.c_double * (2 * K))()
    # slod_lod_inner_ensemble(h, values, ld_m, cols, x, ld_x, y, ld_y, n_members, out, stream)
    _refused(g, "slod_lod_inner_ensemble", [g.h, FAKE, K, FAKE, FAKE, K, FAKE, K, K, out, None],
             ((0, None), (1, None), (3, None), (4, None), (6, None), (9, None),
              (8, 0), (8, -1), (8, 65536),
              (2, K - 1), (5, K - 1), (7, K - 1)))
    # slod_lod_newmark_accel_ensemble_direct(h, f_M, A, ld_a_m, M, ld_m_m, cols, damp_mass, damp_stiff, n_members, u, ld_u,
    #                                        v, ld_v, load, ld_load, a, ld_a): the factor is checked last
    name = "slod_lod_newmark_accel_ensemble_direct"
    ok = [g.h, None, FAKE, K, FAKE, K, FAKE, 0.0, 0.0, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K]
    _refused(g, name, ok,
             ((0, None), (2, None), (4, None), (6, None), (10, None), (12, None), (16, None),   # handle, matrix, cols, state
              (9, 0), (9, -1), (9, 65536),                                                      # n_members
              (3, K - 1), (5, K - 1), (11, K - 1), (13, K - 1), (15, K - 1), (17, K - 1),       # every ld
              (7, -0.1), (7, NANF), (8, -1e-3), (8, NANF)))                                     # damping
    assert g.lib.slod_lod_newmark_accel_ensemble_direct(*ok) == -1
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    ok[14], ok[15] = None, 0                                  # without a load ld_load is not looked at
    assert g.lib.slod_lod_newmark_accel_ensemble_direct(*ok) == -1
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    # slod_lod_newmark_steps_ensemble_direct(h, f_S, A, ld_a_m, M, ld_m_m, cols, dt, beta, gamma, damp_mass, damp_stiff,
    #                                        n_steps, n_members, u, ld_u, v, ld_v, a, ld_a, load, ld_load, stride, kin, pot)
    name = "slod_lod_newmark_steps_ensemble_direct"
    ok = [g.h, None, FAKE, K, FAKE, K, FAKE, 0.01, 0.25, 0.5, 0.0, 0.0, 1, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 0, kin, pot]
    _refused(g, name, ok,
             ((0, None), (2, None), (4, None), (6, None), (14, None), (16, None), (18, None),
              (7, 0.0), (7, -0.01), (7, NANF),                                                  # dt
              (8, 0.6), (8, -0.1), (8, NANF), (9, -0.1), (9, 1.1), (9, NANF),                   # beta, gamma
              (10, -0.1), (10, NANF), (11, -1e-3), (11, NANF),                                  # damping
              (12, 0), (12, -1),                                                                # n_steps
              (13, 0), (13, -1), (13, 65536),                                                   # n_members
              (3, K - 1), (5, K - 1), (15, K - 1), (17, K - 1), (19, K - 1), (21, K - 1),       # every ld
              (23, None), (24, None)))                                                          # one of the energies
    assert g.lib.slod_lod_newmark_steps_ensemble_direct(*ok) == -1
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    ok[20], ok[21], ok[23], ok[24] = None, 0, None, None      # no load, no energies: still the factor
    assert g.lib.slod_lod_newmark_steps_ensemble_direct(*ok) == -1
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    # and through the wrappers: every ld defaults to n_members
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_inner_ensemble(FAKE, FAKE, FAKE, FAKE, K, ld_m=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_accel_ensemble_direct(None, FAKE, FAKE, FAKE, K, FAKE, FAKE, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_accel_ensemble_direct(None, FAKE, FAKE, FAKE, K, FAKE, FAKE, FAKE, ld_m_m=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_steps_ensemble_direct(None, FAKE, FAKE, FAKE, 0.01, 1, K, FAKE, FAKE, FAKE, beta=0.6)
    assert e.value.code == -1 and "beta" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_steps_ensemble_direct(None, FAKE, FAKE, FAKE, 0.01, 1, K, FAKE, FAKE, FAKE, energies=False)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
