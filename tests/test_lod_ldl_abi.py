"""CPU-side checks of the banded LDL^T factor and of the eigensolver near a shift (slod_lod_factor_create_ldl,
slod_lod_factor_create_ldl_ensemble, slod_lod_factor_inertia, slod_lod_eigs_shift_direct,
slod_lod_eigs_shift_ensemble_direct), after the pattern of test_lod_eig_direct_abi.py: the calls are exported, declared
with the signatures of include/slod.h and wrapped, the header documents what it promises, and every SLOD_ERR_ARGUMENT
that needs no factor is returned before any device work (so on a machine without a GPU) with the call's name in
slod_last_error.  The refusals that need a factor (a member out of range, a Cholesky factor given to
slod_lod_factor_inertia, a factor of another member count) are in test_gpu_lod_ldl.py and test_gpu_lod_ldl_eigs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF, INF = float("nan"), float("inf")

# the parameter types of include/slod.h, in order
SIGNATURES = {
    "slod_lod_factor_create_ldl": "slod_handle* double* uint32_t* slod_lod_factor**",
    "slod_lod_factor_create_ldl_ensemble": "slod_handle* double* size_t int uint32_t* int32_t* slod_lod_factor**",
    "slod_lod_factor_inertia": "slod_lod_factor* int slod_lod_factor_inertia_info*",
    "slod_lod_eigs_shift_direct": "slod_handle* slod_lod_factor* double double* double* uint32_t* int int int double* size_t "
                                  "double int double* double*",
    "slod_lod_eigs_shift_ensemble_direct": "slod_handle* slod_lod_factor* double double* size_t double* size_t uint32_t* int "
                                           "int int int double* size_t double int double* double* int*",
}
WRAPPERS = ("lod_factor_ldl", "lod_factor_ldl_ensemble", "lod_eigs_shift_direct", "lod_eigs_shift_ensemble_direct")
SCALARS = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t}


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def _header():
    return open(os.path.join(ROOT, "include", "slod.h")).read()


def _declared_types(name):
    """The parameter types of `name` as include/slod.h declares them: comments and names dropped, const dropped."""
    m = re.search(r"^int %s\((.*?)\);" % name, _header(), re.M | re.S)
    assert m, "not declared: " + name
    out = []
    for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        p = p.replace("const", " ").strip()
        words = p.replace("*", " ").split()
        out.append(" ".join(words[:-1]) + "*" * p.count("*"))
    return out


def test_lod_ldl_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n, sig in SIGNATURES.items():
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = sig.split()
        assert _declared_types(n) == want, (n, _declared_types(n))
        got = getattr(lib, n).argtypes                       # the binding passes what the header declares
        assert len(got) == len(want), n
        for t, w in zip(got, want):
            if w.endswith("*"):
                assert t is C.c_void_p or issubclass(t, C._Pointer), (n, w, t)
            else:
                assert t is SCALARS[w], (n, w, t)
    assert lib.slod_abi_version() == 5
    for m in WRAPPERS:
        assert callable(getattr(slod_amd.Slod, m))
    assert callable(slod_amd.LodFactor.inertia) and slod_amd.LodFactor is slod_amd.Factor


def test_inertia_struct_matches_the_header():
    """The fields of slod_lod_factor_inertia_info in the order and with the types of the binding's structure."""
    import slod_amd
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*slod_lod_factor_inertia_info;", _header(), re.S)
    assert m
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        words = decl.replace(",", " ").split()
        fields += [(w, words[0]) for w in words[1:]]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctype[t]) for n, t in fields] == list(slod_amd.InertiaInfo._fields_)
    assert C.sizeof(slod_amd.InertiaInfo) == 40


def test_header_documents_the_ldl_factor():
    flat = " ".join(_header().split())
    for promised in ("promised to a factor of 2",                         # norm_factor is a diagnostic
                     "1 / (b eps)",                                       # the growth beyond which the shift should move
                     "takes an LDL^T factor unchanged",                   # the consumers
                     "the smallest and largest entry of D, signed",       # get_info on an LDL^T factor
                     "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",   # the hashed start block
                     "is zero or not finite"):
        assert promised in flat, promised
    assert "Not built: LDL^T" not in flat and "LDL^T and eigenvalues near an interior sigma" not in flat


def test_hash_block_formula_in_numpy():
    """The formula of the header in uint64 arithmetic: values in [-1, 1), distinct columns, the same on every call."""
    from lod_ldl_cases import hash_block
    X = hash_block(25, 8)
    assert X.shape == (25, 8) and (X >= -1.0).all() and (X < 1.0).all()
    assert np.linalg.matrix_rank(X) == 8
    mask = (1 << 64) - 1                                                  # the same entry in Python's integers
    z = ((3 << 32 | 5) + 0x9E3779B97F4A7C15) & mask
    z = ((z ^ z >> 30) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ z >> 27) * 0x94D049BB133111EB) & mask
    z ^= z >> 31
    assert X[3, 5] == float(z >> 11) * 2.0 ** -52 - 1.0


def _refused(g, name, ok, cases, fix=None):
    """Every (position, bad value) alone makes the call return SLOD_ERR_ARGUMENT and leaves the call's name in the
    handle's error text (a NULL handle leaves it in the thread's, or nothing)."""
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        if fix:
            fix(a, at, bad)
        assert f(*a) == -1, (name, at, bad)
        if at != 0:
            msg = g.lib.slod_last_error(g.h).decode()
            assert name + ":" in msg and "NULL factor" not in msg, (name, at, bad, msg)


def test_lod_ldl_factor_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1, n_problems=3)
    K = 3
    out = C.c_void_p(1)
    bad = (C.c_int32 * K)()
    ref = C.byref(out)
    _refused(g, "slod_lod_factor_create_ldl", [g.h, FAKE, FAKE, ref], ((0, None), (1, None), (2, None), (3, None)))
    assert out.value is None                                             # *out is cleared before the checks
    _refused(g, "slod_lod_factor_create_ldl_ensemble", [g.h, FAKE, K, K, FAKE, bad, ref],
             ((0, None), (1, None), (4, None), (6, None), (3, 0), (3, -1), (3, 65536), (2, K - 1)))
    info = slod_amd.InertiaInfo()
    assert g.lib.slod_lod_factor_inertia(None, 0, C.byref(info)) == -1
    assert g.lib.slod_lod_factor_inertia(FAKE, 0, None) == -1           # refused before the factor is read
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_ldl(None, FAKE)
    assert e.value.code == -1 and "slod_lod_factor_create_ldl:" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_ldl_ensemble(FAKE, FAKE, K, ld_m=K - 1)
    assert e.value.code == -1 and "slod_lod_factor_create_ldl_ensemble:" in str(e.value) and "leading dimension" in str(e.value)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_eigs_shift_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    rows = g.num_patches * spacedim           # 16 or 32: below the cap of 64 columns
    m, K = 6, 3
    lam, res = (C.c_double * (64 * K))(), (C.c_double * (64 * K))()
    status = (C.c_int * K)()
    # slod_lod_eigs_shift_direct(h, f_S, sigma, A, M, cols, n_eig, n_block, start, x, ld_x, tol, max_outer, eigenvalues,
    #                            residuals)
    name = "slod_lod_eigs_shift_direct"
    ok = [g.h, None, 3.5, FAKE, FAKE, FAKE, 2, m, 0, FAKE, m, 1e-10, 5, lam, res]

    def wide(a, at, bad):                                               # so that only n_block is wrong
        if at == 7 and bad > m:
            a[10] = bad

    _refused(g, name, ok,
             ((0, None), (3, None), (4, None), (5, None), (9, None), (13, None), (14, None),
              (2, NANF), (2, INF), (2, -INF),                             # sigma
              (6, 0), (6, -1), (6, m + 1),                                # n_eig < 1, n_block < n_eig
              (7, 65), (7, rows + 1),                                     # n_block > 64, > rows
              (10, m - 1),                                                # ld_x < n_block
              (8, 2), (8, -1),                                            # start
              (11, 0.0), (11, -1e-10), (11, NANF),                        # tol
              (12, 0), (12, -1)), fix=wide)                               # max_outer
    assert g.lib.slod_lod_eigs_shift_direct(*ok) == -1                   # all good but the factor: it is checked last
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    # slod_lod_eigs_shift_ensemble_direct(h, f_S, sigma, A, ld_a_m, M, ld_m_m, cols, n_members, n_eig, n_block, start, x,
    #                                     ld_x, tol, max_outer, eigenvalues, residuals, member_status)
    name = "slod_lod_eigs_shift_ensemble_direct"
    ok = [g.h, None, -2.0, FAKE, K, FAKE, K + 1, FAKE, K, 2, m, 0, FAKE, K * m, 1e-10, 5, lam, res, status]

    def wide_ens(a, at, bad):
        if at == 10 and bad > m:
            a[13] = K * bad

    _refused(g, name, ok,
             ((0, None), (3, None), (5, None), (7, None), (12, None), (16, None), (17, None),
              (18, None),                                                 # member_status
              (2, NANF), (2, INF),
              (9, 0), (9, -1), (9, m + 1),
              (10, 65), (10, rows + 1),
              (11, 2), (11, -1),
              (14, 0.0), (14, -1e-10), (14, NANF),
              (15, 0), (15, -1),
              (8, 0), (8, -1), (8, 65536),                                # n_members
              (4, K - 1), (6, K - 1),                                     # a matrix ld below n_members
              (13, K * m - 1), (13, m)), fix=wide_ens)                    # ld_x < n_members * n_block
    assert g.lib.slod_lod_eigs_shift_ensemble_direct(*ok) == -1
    assert name + ": NULL factor" in g.lib.slod_last_error(g.h).decode()
    # and through the wrappers: every ld has its default
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_shift_direct(None, 1.0, FAKE, FAKE, FAKE, 2, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_shift_direct(None, NANF, FAKE, FAKE, FAKE, 2, FAKE)
    assert e.value.code == -1 and "sigma" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_shift_ensemble_direct(None, 1.0, FAKE, FAKE, FAKE, K, 2, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs_shift_ensemble_direct(None, 1.0, FAKE, FAKE, FAKE, K, 2, FAKE, n_block=m, ld_x=K * m - 1)
    assert e.value.code == -1 and "n_members * n_block" in str(e.value)
