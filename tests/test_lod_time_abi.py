"""CPU-side checks of the mass matrix, the block-row product and combination, and the theta stepper
(slod_lod_mass_matrix, slod_lod_apply_multi, slod_lod_matrix_combine, slod_lod_theta_steps): they are exported and
declared, their argument checks come before any device work (so they answer on a machine without a GPU), and
without a GPU the calls fail loudly."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("slod_lod_mass_matrix", "slod_lod_apply_multi", "slod_lod_matrix_combine", "slod_lod_theta_steps")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_time_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in ("lod_mass_matrix", "lod_apply", "lod_matrix_combine", "lod_theta_steps"):
        assert callable(getattr(slod_amd.Slod, m))


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_time_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim)
    lib = g.lib
    rows = np.arange(g.num_patches, dtype=np.uint32)
    rp = rows.ctypes.data_as(C.POINTER(C.c_uint32))
    bad_rows = np.array([0, g.num_patches], dtype=np.uint32)
    n, K, steps = len(rows), 3, 4
    its = (C.c_int * steps)()
    res = (C.c_double * steps)()
    # slod_lod_mass_matrix(h, rows, n_rows, basis, stride, rho, values, cols, stream); rho may be NULL
    ok = [g.h, rp, n, FAKE, 64, None, FAKE, FAKE, None]
    for at, bad in ((0, None), (1, None), (3, None), (6, None), (7, None),
                    (1, bad_rows.ctypes.data_as(C.POINTER(C.c_uint32)))):      # a row id out of range
        a = list(ok)
        a[at] = bad
        if at == 1 and bad is not None:
            a[2] = 2
        assert lib.slod_lod_mass_matrix(*a) == -1, (at, bad)
    assert "slod_lod_mass_matrix" in lib.slod_last_error(g.h).decode()
    # slod_lod_apply_multi(h, values, cols, x, ld_x, n_rhs, y, ld_y, stream)
    ok = [g.h, FAKE, FAKE, FAKE, K, K, 2 * FAKE, K, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (6, None),
                    (5, 0), (5, -1),                                        # n_rhs < 1
                    (4, K - 1), (7, K - 1),                                 # ld_x, ld_y < n_rhs
                    (6, FAKE)):                                             # in place
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_apply_multi(*a) == -1, (at, bad)
    assert "slod_lod_apply_multi" in lib.slod_last_error(g.h).decode()
    # slod_lod_matrix_combine(h, alpha, a, beta, b, out, stream)
    ok = [g.h, 1.0, FAKE, 0.5, FAKE, FAKE, None]
    for at in (0, 2, 4, 5):
        a = list(ok)
        a[at] = None
        assert lib.slod_lod_matrix_combine(*a) == -1, at
    # slod_lod_theta_steps(h, stiffness, mass, cols, dt, theta, n_steps, n_rhs, u, ld_u, load, ld_load, stride,
    #                      tol, maxit, iterations, residual)
    ok = [g.h, FAKE, FAKE, FAKE, 0.01, 1.0, steps, K, FAKE, K, FAKE, K, 0, 1e-12, 10, its, res]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (8, None),   # NULL handle, matrices, cols, state
                    (4, 0.0), (4, -0.01), (4, float("nan")),                # dt <= 0
                    (5, -0.1), (5, 1.1), (5, float("nan")),                 # theta outside [0, 1]
                    (6, 0), (6, -1),                                        # n_steps < 1
                    (7, 0), (7, -1),                                        # n_rhs < 1
                    (9, K - 1), (11, K - 1),                                # ld_u, ld_load < n_rhs
                    (14, -1)):                                              # max_iterations < 0
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_theta_steps(*a) == -1, (at, bad)
    assert "slod_lod_theta_steps" in lib.slod_last_error(g.h).decode()
    # and through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_theta_steps(FAKE, FAKE, FAKE, 0.01, 1.5, 1, FAKE)
    assert e.value.code == -1 and "theta" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_apply(FAKE, FAKE, FAKE, 2 * FAKE, n_rhs=K, ld_x=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_mass_matrix(bad_rows, FAKE, 64, FAKE, FAKE)
    assert e.value.code == -1 and "out of range" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_combine(1.0, None, 1.0, FAKE, FAKE)
    assert e.value.code == -1


def test_lod_time_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    rows = np.arange(g.num_patches, dtype=np.uint32)
    calls = (lambda: g.lod_mass_matrix(rows, FAKE, 64, FAKE, FAKE),
             lambda: g.lod_apply(FAKE, FAKE, FAKE, 2 * FAKE, n_rhs=2),
             lambda: g.lod_matrix_combine(1.0, FAKE, 0.5, FAKE, FAKE),
             lambda: g.lod_theta_steps(FAKE, FAKE, FAKE, 0.01, 1.0, 2, FAKE, n_rhs=2),
             lambda: g.lod_theta_steps(FAKE, FAKE, FAKE, 0.01, 0.5, 2, FAKE, d_load=FAKE, load_step_stride=64))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
