"""CPU-side checks of the multi-vector LOD entry points (slod_lod_rhs_multi, slod_lod_solve_multi,
slod_lod_reconstruct_multi): they are exported and declared, their argument checks come before any device work
(so they answer on a machine without a GPU), and without a GPU the calls fail loudly."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("slod_lod_rhs_multi", "slod_lod_solve_multi", "slod_lod_reconstruct_multi")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_multi_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in ("lod_rhs_multi", "lod_solve_multi", "lod_reconstruct_multi"):
        assert callable(getattr(slod_amd.Slod, m))


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_multi_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim)
    lib = g.lib
    rows = np.arange(g.num_patches, dtype=np.uint32)
    rp = rows.ctypes.data_as(C.POINTER(C.c_uint32))
    n, K = len(rows), 3
    field = (g.NE + 1) ** 2 * spacedim
    its = (C.c_int * K)()
    res = (C.c_double * K)()
    # slod_lod_rhs_multi(h, rows, n_rows, basis, stride, fine, ld_fine, n_rhs, out, ld_out, stream)
    ok = [g.h, rp, n, FAKE, 64, FAKE, field, K, FAKE, K, None]
    for at, bad in ((0, None), (1, None), (3, None), (5, None), (8, None),   # NULL handle / arrays
                    (7, 0), (7, -2),                                        # n_rhs < 1
                    (9, K - 1),                                             # ld_out < n_rhs
                    (6, field - 1)):                                        # ld_fine shorter than a field
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_rhs_multi(*a) == -1, (at, bad)
    assert "slod_lod_rhs_multi" in lib.slod_last_error(g.h).decode()
    # slod_lod_solve_multi(h, values, cols, rhs, ld_rhs, n_rhs, u, ld_u, tol, maxit, iterations, residual)
    ok = [g.h, FAKE, FAKE, FAKE, K, K, FAKE, K, 1e-12, 10, its, res]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (6, None),
                    (5, 0), (5, -1),
                    (4, K - 1), (7, K - 1),                                 # ld_rhs, ld_u < n_rhs
                    (9, -1)):                                               # max_iterations < 0
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_solve_multi(*a) == -1, (at, bad)
    assert "slod_lod_solve_multi" in lib.slod_last_error(g.h).decode()
    # slod_lod_reconstruct_multi(h, basis, stride, u, ld_u, n_rhs, fine, ld_fine, stream)
    ok = [g.h, FAKE, 64, FAKE, K, K, FAKE, field, None]
    for at, bad in ((0, None), (1, None), (3, None), (6, None),
                    (5, 0), (5, -1),
                    (4, K - 1),
                    (7, field - 1)):
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_reconstruct_multi(*a) == -1, (at, bad)
    assert "slod_lod_reconstruct_multi" in lib.slod_last_error(g.h).decode()
    # and through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_multi(FAKE, FAKE, FAKE, K - 1, K, FAKE, K)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_rhs_multi(rows, FAKE, 64, FAKE, field, 0, FAKE, K)
    assert e.value.code == -1
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_reconstruct_multi(FAKE, 64, FAKE, K, K, FAKE, field - 1)
    assert e.value.code == -1 and "ld_fine" in str(e.value)


def test_lod_multi_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    rows = np.arange(g.num_patches, dtype=np.uint32)
    field = (g.NE + 1) ** 2
    calls = (lambda: g.lod_rhs_multi(rows, FAKE, 64, FAKE, field, 2, FAKE, 2),
             lambda: g.lod_solve_multi(FAKE, FAKE, FAKE, 2, 2, FAKE, 2),
             lambda: g.lod_reconstruct_multi(FAKE, 64, FAKE, 2, 2, FAKE, field))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
