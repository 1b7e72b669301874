"""CPU-side checks of the eigensolver on banded Cholesky factors (slod_lod_eigs_direct, slod_lod_eigs_ensemble_direct):
the calls are exported, declared with the signatures of include/slod.h and wrapped, and every SLOD_ERR_ARGUMENT that
needs no factor is returned before any device work (so it is returned on a machine without a GPU) with the call's name
in slod_last_error.  The factor is checked last, so a NULL factor behind good arguments is the "NULL factor" refusal.
The refusals that need a factor (another handle or row count, another member count, the single call on a factor of
several members) are in test_gpu_lod_eig_direct.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slod_lod_eigs_direct", "slod_lod_eigs_ensemble_direct")
WRAPPERS = ("lod_eigs_direct", "lod_eigs_ensemble_direct")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF = float("nan")

# the parameter types of include/slod.h, in order
SIGNATURES = {
    "slod_lod_eigs_direct": "slod_handle* slod_lod_factor* double* double* uint32_t* int int int double* size_t double int "
                            "double* double*",
    "slod_lod_eigs_ensemble_direct": "slod_handle* slod_lod_factor* double* size_t double* size_t uint32_t* int int int int "
                                     "double* size_t double int double* double* int*",
}
CTYPES = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t, "double*": (C.c_void_p, C.POINTER(C.c_double)),
          "int*": (C.c_void_p, C.POINTER(C.c_int))}


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


def test_lod_eig_direct_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = SIGNATURES[n].split()
        assert _declared_types(n) == want, (n, _declared_types(n))
        got = getattr(lib, n).argtypes                       # the binding passes what the header declares
        assert len(got) == len(want), n
        for t, w in zip(got, want):
            if w.endswith("*"):
                assert t in CTYPES.get(w, (C.c_void_p,)), (n, w, t)
            else:
                assert t is CTYPES[w], (n, w, t)
    assert lib.slod_abi_version() == 5
    for m in WRAPPERS:
        assert callable(getattr(slod_amd.Slod, m))


def test_not_built_lists_no_longer_name_what_is_built():
    """The header and DESIGN keep LDL^T, interior shifts, LOBPCG, locking and n_block > 64 as not built, and no longer
    the ensemble eigensolver or the eigensolver's inner solve on a factor."""
    header = open(os.path.join(ROOT, "include", "slod.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (header, design):
        flat = " ".join(text.split())
        assert "the ensemble eigensolver" not in flat
        assert "the eigensolver's inner solve on a factor" not in flat
    flat = " ".join(header.split())
    for kept in ("LDL^T", "LOBPCG", "locking", "n_block > 64"):
        assert kept in flat, kept


def _refused(g, name, ok, cases, fix=None):
    """Every (position, bad value) alone makes the call return SLOD_ERR_ARGUMENT and leaves the call's name in the
    handle's error text (a NULL handle leaves it in the thread's)."""
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        if fix:
            fix(a, at, bad)
        assert f(*a) == -1, (name, at, bad)
        msg = g.lib.slod_last_error(None if at == 0 else g.h).decode()
        assert name + ":" in msg and "NULL factor" not in msg, (name, at, bad, msg)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_eig_direct_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    rows = g.num_patches * spacedim           # 16 or 32: below the cap of 64 columns
    m, K = 6, 3
    lam, res = (C.c_double * (64 * K))(), (C.c_double * (64 * K))()
    status = (C.c_int * K)()
    # slod_lod_eigs_direct(h, f_S, A, M, cols, n_eig, n_block, start, x, ld_x, tol, max_outer, eigenvalues, residuals)
    name = "slod_lod_eigs_direct"
    ok = [g.h, None, FAKE, FAKE, FAKE, 2, m, 0, FAKE, m, 1e-10, 5, lam, res]

    def wide(a, at, bad):                                               # so that only n_block is wrong
        if at == 6 and bad > m:
            a[9] = bad

    _refused(g, name, ok,
             ((0, None), (2, None), (3, None), (4, None), (8, None), (12, None), (13, None),
              (5, 0), (5, -1), (5, m + 1),                                # n_eig < 1, n_block < n_eig
              (6, 65), (6, rows + 1),                                     # n_block > 64, > rows
              (9, m - 1),                                                 # ld_x < n_block
              (7, 2), (7, -1),                                            # start
              (10, 0.0), (10, -1e-10), (10, NANF),                        # tol
              (11, 0), (11, -1)), fix=wide)                               # max_outer
    assert g.lib.slod_lod_eigs_direct(*ok) == -1                         # all good but the factor: it is checked last
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    # slod_lod_eigs_ensemble_direct(h, f_S, A, ld_a_m, M, ld_m_m, cols, n_members, n_eig, n_block, start, x, ld_x, tol,
    #                               max_outer, eigenvalues, residuals, member_status)
    name = "slod_lod_eigs_ensemble_direct"
    ok = [g.h, None, FAKE, K, FAKE, K + 1, FAKE, K, 2, m, 0, FAKE, K * m, 1e-10, 5, lam, res, status]

    def wide_ens(a, at, bad):
        if at == 9 and bad > m:
            a[12] = K * bad

    _refused(g, name, ok,
             ((0, None), (2, None), (4, None), (6, None), (11, None), (15, None), (16, None),
              (17, None),                                                 # member_status
              (8, 0), (8, -1), (8, m + 1),
              (9, 65), (9, rows + 1),
              (10, 2), (10, -1),
              (13, 0.0), (13, -1e-10), (13, NANF),
              (14, 0), (14, -1),
              (7, 0), (7, -1), (7, 65536),                                # n_members
              (3, K - 1), (5, K - 1),                                     # a matrix ld below n_members
              (12, K * m - 1), (12, m)), fix=wide_ens)                    # ld_x < n_members * n_block
    assert g.lib.slod_lod_eigs_ensemble_direct(*ok) == -1
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    # and through the wrappers: every ld has its default
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_direct(None, FAKE, FAKE, FAKE, 2, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_direct(None, FAKE, FAKE, FAKE, 2, FAKE, n_block=65, ld_x=65)
    assert e.value.code == -1 and "n_block" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_ensemble_direct(None, FAKE, FAKE, FAKE, K, 2, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_ensemble_direct(None, FAKE, FAKE, FAKE, K, 2, FAKE, ld_m_m=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_ensemble_direct(None, FAKE, FAKE, FAKE, K, 2, FAKE, n_block=m, ld_x=K * m - 1)
    assert e.value.code == -1 and "n_members * n_block" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_ensemble_direct(None, FAKE, FAKE, FAKE, 65536, 2, FAKE)
    assert e.value.code == -1 and "n_members" in str(e.value)
