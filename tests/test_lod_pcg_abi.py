"""CPU-side checks of CG preconditioned by a banded factor (slod_lod_solve_multi_precond, slod_lod_solve_ensemble_precond):
the calls are exported, declared with the signatures of include/slod.h and wrapped, and every SLOD_ERR_ARGUMENT that needs
no factor is returned before any device work (so it is returned on a machine without a GPU) with the call's name in
slod_last_error, the NULL handle included.  The factor is checked last, so a NULL factor behind good arguments is the
"NULL factor" refusal in the words of slod_lod_factor_check.  A factor cannot exist without a device, so the refusals that
need one (another handle, another member count, an LDL^T factor with a negative pivot) and SLOD_ERR_DEVICE behind a good
factor are out of reach here: the former are in test_gpu_lod_pcg.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slod_lod_solve_multi_precond", "slod_lod_solve_ensemble_precond")
WRAPPERS = ("lod_solve_multi_precond", "lod_solve_ensemble_precond")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
SIGNATURES = {
    "slod_lod_solve_multi_precond": "slod_handle* slod_lod_factor* double* uint32_t* double* size_t int double* size_t double int "
                                    "int* double*",
    "slod_lod_solve_ensemble_precond": "slod_handle* slod_lod_factor* double* size_t uint32_t* double* size_t int double* size_t "
                                       "double int int* double*",
}
CTYPES = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t, "double*": (C.c_void_p, C.POINTER(C.c_double)),
          "int*": (C.c_void_p, C.POINTER(C.c_int))}


def _declared_types(name):
    """The parameter types of `name` as include/slod.h declares them: comments and names dropped, const dropped."""
    text = open(os.path.join(ROOT, "include", "slod.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S)
    assert m, "not declared: " + name
    out = []
    for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        p = p.replace("const", " ").strip()
        out.append(" ".join(p.replace("*", " ").split()[:-1]) + "*" * p.count("*"))
    return out


def test_lod_pcg_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = SIGNATURES[n].split()
        assert _declared_types(n) == want, (n, _declared_types(n))
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
    f = getattr(g.lib, name)
    for at, bad, word in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        msg = g.lib.slod_last_error(None if at == 0 else g.h).decode()
        assert name + ":" in msg and word in msg and "NULL factor" not in msg, (name, at, bad, msg)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_pcg_argument_checks(spacedim):
    import slod_amd
    g = slod_amd.Slod(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    K = 3
    its, res = (C.c_int * 8)(), (C.c_double * 8)()
    # slod_lod_solve_multi_precond(h, f_P, values, cols, rhs, ld_rhs, n_rhs, u, ld_u, rel_tol, max_iterations, its, res)
    name = "slod_lod_solve_multi_precond"
    ok = [g.h, None, FAKE, FAKE, FAKE, 5, 5, FAKE, 6, 1e-10, 10, its, res]
    _refused(g, name, ok,
             ((0, None, "NULL handle or array"), (2, None, "NULL handle or array"), (3, None, "NULL handle or array"),
              (4, None, "NULL handle or array"), (7, None, "NULL handle or array"),
              (6, 0, "n_rhs < 1"), (6, -2, "n_rhs < 1"), (10, -1, "max_iterations < 0"),
              (5, 4, "leading dimension below n_rhs"), (8, 4, "leading dimension below n_rhs")))
    for a in (ok, ok[:11] + [None, None]):                               # all good but the factor: it is checked last
        assert g.lib.slod_lod_solve_multi_precond(*a) == -1
        assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    # slod_lod_solve_ensemble_precond(h, f_P, values, ld_m, cols, rhs, ld_rhs, n_members, u, ld_u, rel_tol, max_it, its, res)
    name = "slod_lod_solve_ensemble_precond"
    ok = [g.h, None, FAKE, K, FAKE, FAKE, K + 1, K, FAKE, K + 2, 1e-10, 10, its, res]
    _refused(g, name, ok,
             ((0, None, "NULL handle or array"), (2, None, "NULL handle or array"), (4, None, "NULL handle or array"),
              (5, None, "NULL handle or array"), (8, None, "NULL handle or array"),
              (7, 0, "n_members < 1"), (7, -1, "n_members < 1"), (11, -1, "max_iterations < 0"),
              (3, K - 1, "leading dimension below n_members"), (6, K - 1, "leading dimension below n_members"),
              (9, K - 1, "leading dimension below n_members")))
    assert g.lib.slod_lod_solve_ensemble_precond(*ok) == -1
    assert g.lib.slod_last_error(g.h).decode() == name + ": NULL factor"
    # and through the wrappers: every ld of the ensemble call has its default
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_multi_precond(None, FAKE, FAKE, FAKE, 5, 5, FAKE, 5)
    assert e.value.code == -1 and "NULL factor" in str(e.value) and len(e.value.iterations) == 5
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_multi_precond(None, FAKE, FAKE, FAKE, 4, 5, FAKE, 5)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_ensemble_precond(None, FAKE, FAKE, FAKE, FAKE, K)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_ensemble_precond(None, FAKE, FAKE, FAKE, FAKE, K, ld_m=K - 1)
    assert e.value.code == -1 and "leading dimension below n_members" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_ensemble_precond(None, FAKE, FAKE, FAKE, FAKE, 0)
    assert e.value.code == -1 and "n_members" in str(e.value)
    g.close()
