"""CPU-side checks of the symmetrisation and the eigensolver of the LOD pencil (slod_lod_matrix_symmetrize,
slod_lod_eigs): they are exported and declared, their argument checks come before any device work (so they answer
on a machine without a GPU), and without a GPU the calls fail loudly."""
import ctypes as C

import pytest

NAMES = ("slod_lod_matrix_symmetrize", "slod_lod_eigs")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NAN = float("nan")


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_eig_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in ("lod_matrix_symmetrize", "lod_eigs"):
        assert callable(getattr(slod_amd.Slod, m))


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_eig_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim)
    lib = g.lib
    rows = g.num_patches * spacedim           # 16 or 32: below the cap of 64 columns
    m, outer = 6, 5
    lam = (C.c_double * 64)()
    res = (C.c_double * 64)()
    its = (C.c_int * outer)()
    # slod_lod_matrix_symmetrize(h, values, cols, out, stream)
    ok = [g.h, FAKE, FAKE, 2 * FAKE, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (3, FAKE)):      # NULL arguments; in place
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_matrix_symmetrize(*a) == -1, (at, bad)
    assert "slod_lod_matrix_symmetrize" in lib.slod_last_error(g.h).decode()
    # slod_lod_eigs(h, stiffness, mass, cols, n_eig, n_block, start, x, ld_x, tol, max_outer, inner_tol, inner_maxit,
    #               eigenvalues, residuals, inner_iterations)
    ok = [g.h, FAKE, FAKE, FAKE, 2, m, 0, FAKE, m, 1e-10, outer, 1e-12, 100, lam, res, its]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (7, None), (13, None), (14, None),
                    (4, 0), (4, -1),                                        # n_eig < 1
                    (4, m + 1),                                             # n_block < n_eig
                    (5, 65), (5, rows + 1),                                 # n_block > 64, n_block > rows
                    (8, m - 1),                                             # ld_x < n_block
                    (6, 2), (6, -1),                                        # start not in {0, 1}
                    (9, 0.0), (9, -1e-10), (9, NAN),                        # tol
                    (11, 0.0), (11, -1e-12), (11, NAN),                     # inner_rel_tol
                    (10, 0), (10, -1),                                      # max_outer < 1
                    (12, -1)):                                              # inner_max_iterations < 0
        a = list(ok)
        a[at] = bad
        if (at, bad) == (5, 65):
            a[8] = 65                                                       # so that only n_block is wrong
        if (at, bad) == (5, rows + 1):
            a[8] = rows + 1
        assert lib.slod_lod_eigs(*a) == -1, (at, bad)
        if at not in (0, 1, 2, 3, 7, 13, 14):
            assert "slod_lod_eigs" in lib.slod_last_error(g.h).decode(), (at, bad)
    # inner_iterations may be NULL: with good arguments the call goes on to the device
    import torch
    if not torch.cuda.is_available():
        a = list(ok)
        a[15] = None
        assert lib.slod_lod_eigs(*a) == -3
    # and through the wrappers
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_symmetrize(FAKE, FAKE, FAKE)
    assert e.value.code == -1 and "in place" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs(FAKE, FAKE, FAKE, 2, FAKE, n_block=65, ld_x=65)
    assert e.value.code == -1 and "n_block" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs(FAKE, FAKE, FAKE, 2, FAKE, start=3)
    assert e.value.code == -1 and "start" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs(FAKE, FAKE, FAKE, 2, FAKE, tol=NAN)
    assert e.value.code == -1 and "tol" in str(e.value)


def test_lod_eigs_default_block_width():
    """n_block defaults to min(64, rows, n_eig + max(4, n_eig // 2)): with 16 rows, n_eig = 14 asks for 16 columns and
    passes the checks (no GPU: -3, not -1), which n_block = 21 would not."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_eigs(FAKE, FAKE, FAKE, 14, FAKE)
    assert e.value.code == -3


def test_lod_eig_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    calls = (lambda: g.lod_matrix_symmetrize(FAKE, FAKE, 2 * FAKE),
             lambda: g.lod_eigs(FAKE, FAKE, FAKE, 2, FAKE),
             lambda: g.lod_eigs(FAKE, FAKE, FAKE, 1, FAKE, n_block=1, start=1, ld_x=4))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
