"""CPU-side checks of the ensemble block (slod_lod_matrix_ensemble, slod_lod_rhs_ensemble, slod_lod_apply_ensemble,
slod_lod_solve_ensemble, slod_lod_reconstruct_ensemble, slod_ensemble_moments): the calls are exported, declared and
wrapped, their argument checks come before any device work (so they answer on a machine without a GPU) and name the
call, and without a GPU the calls fail loudly."""
import ctypes as C

import pytest

NAMES = ("slod_lod_matrix_ensemble", "slod_lod_rhs_ensemble", "slod_lod_apply_ensemble", "slod_lod_solve_ensemble",
         "slod_lod_reconstruct_ensemble", "slod_ensemble_moments")
WRAPPERS = ("lod_matrix_ensemble", "lod_rhs_ensemble", "lod_apply_ensemble", "lod_solve_ensemble",
            "lod_reconstruct_ensemble", "ensemble_moments")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_ensemble_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
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
def test_lod_ensemble_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    K, NP = 3, g.num_patches
    stride = 4096                                  # any slab stride: nothing is dereferenced
    slab = NP * stride
    field = (g.NE + 1) ** 2 * spacedim
    its = (C.c_int * K)()
    res = (C.c_double * K)()
    # slod_lod_matrix_ensemble(h, basis, premult, stride, member_stride, n_members, values, ld_m, cols, stream)
    _refused(g, "slod_lod_matrix_ensemble", [g.h, FAKE, FAKE, stride, slab, K, FAKE, K, FAKE, None],
             ((0, None), (1, None), (2, None), (6, None), (8, None),      # NULL handle or array
              (5, 0), (5, -1), (5, 65536),                                # n_members < 1 or beyond a grid axis
              (7, K - 1),                                                 # ld_m < n_members
              (4, slab - 1), (4, 0)))                                     # member_stride shorter than a slab
    # slod_lod_rhs_ensemble(h, basis, stride, member_stride, n_members, fine_rhs, ld_fine, out, ld_out, stream)
    _refused(g, "slod_lod_rhs_ensemble", [g.h, FAKE, stride, slab, K, FAKE, 0, FAKE, K, None],
             ((0, None), (1, None), (5, None), (7, None),
              (4, 0), (4, -1),
              (8, K - 1),                                                 # ld_out
              (3, slab - 1),
              (6, field - 1), (6, 1)))                                    # ld_fine non-zero but shorter than a field
    # slod_lod_apply_ensemble(h, values, ld_m, cols, x, ld_x, n_members, y, ld_y, stream)
    _refused(g, "slod_lod_apply_ensemble", [g.h, FAKE, K, FAKE, FAKE, K, K, 2 * FAKE, K, None],
             ((0, None), (1, None), (3, None), (4, None), (7, None),
              (6, 0), (6, -1),
              (2, K - 1), (5, K - 1), (8, K - 1),                         # ld_m, ld_x, ld_y
              (7, FAKE)))                                                 # d_x == d_y
    # slod_lod_solve_ensemble(h, values, ld_m, cols, rhs, ld_rhs, n_members, u, ld_u, tol, maxit, iterations, residual)
    _refused(g, "slod_lod_solve_ensemble", [g.h, FAKE, K, FAKE, FAKE, K, K, FAKE, K, 1e-10, 10, its, res],
             ((0, None), (1, None), (3, None), (4, None), (7, None),
              (6, 0), (6, -1),
              (2, K - 1), (5, K - 1), (8, K - 1),                         # ld_m, ld_rhs, ld_u
              (10, -1)))                                                  # max_iterations < 0
    # slod_lod_reconstruct_ensemble(h, basis, stride, member_stride, n_members, u, ld_u, fine, ld_fine, stream)
    _refused(g, "slod_lod_reconstruct_ensemble", [g.h, FAKE, stride, slab, K, FAKE, K, FAKE, field, None],
             ((0, None), (1, None), (5, None), (7, None),
              (4, 0), (4, -1),
              (6, K - 1),                                                 # ld_u
              (3, slab - 1),
              (8, field - 1), (8, 0)))                                    # ld_fine shorter than a field
    # slod_ensemble_moments(h, fields, ld_fine, n_members, count, mean, var, stream)
    _refused(g, "slod_ensemble_moments", [g.h, FAKE, 101, K, 101, FAKE, None, None],
             ((0, None), (1, None), (5, None),
              (3, 0), (3, -1),
              (4, 0),                                                     # count = 0
              (2, 100)))                                                  # ld_fine shorter than a field
    # and through the wrappers
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_ensemble(FAKE, FAKE, stride, K, FAKE, FAKE, ld_m=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_rhs_ensemble(FAKE, stride, K, FAKE, FAKE, member_stride=slab - 1)
    assert e.value.code == -1 and "member_stride" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_apply_ensemble(FAKE, FAKE, FAKE, FAKE, K)
    assert e.value.code == -1 and "in place" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_solve_ensemble(FAKE, FAKE, FAKE, FAKE, K, max_iterations=-1)
    assert e.value.code == -1 and "max_iterations" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_reconstruct_ensemble(FAKE, stride, K, FAKE, FAKE, ld_fine=field - 1)
    assert e.value.code == -1 and "ld_fine" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.ensemble_moments(FAKE, K, 0, FAKE)
    assert e.value.code == -1 and "count" in str(e.value)


def test_lod_ensemble_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, n_problems=2)
    K, stride = 2, 4096
    calls = (lambda: g.lod_matrix_ensemble(FAKE, FAKE, stride, K, FAKE, FAKE),
             lambda: g.lod_rhs_ensemble(FAKE, stride, K, FAKE, FAKE),
             lambda: g.lod_apply_ensemble(FAKE, FAKE, FAKE, 2 * FAKE, K),
             lambda: g.lod_solve_ensemble(FAKE, FAKE, FAKE, FAKE, K),
             lambda: g.lod_reconstruct_ensemble(FAKE, stride, K, FAKE, FAKE),
             lambda: g.ensemble_moments(FAKE, K, 16, FAKE))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
