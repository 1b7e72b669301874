"""CPU-side checks of ensemble time stepping on banded Cholesky factors (slod_lod_mass_matrix_ensemble,
slod_lod_matrix_symmetrize_ensemble, slod_lod_matrix_combine_ensemble, slod_lod_factor_create_ensemble,
slod_lod_factor_get_info_member, slod_lod_factor_solve_ensemble, slod_lod_theta_steps_ensemble_direct): the calls are
exported, declared and wrapped, every SLOD_ERR_ARGUMENT the header lists that needs no factor is returned before any
device work (so it is returned on a machine without a GPU) with the call's name in slod_last_error, and without a GPU
the calls fail loudly.  The refusals that need a factor (another member count, members outside the factor) are in
test_gpu_lod_ensemble_direct.py."""
import ctypes as C

import pytest

NAMES = ("slod_lod_mass_matrix_ensemble", "slod_lod_matrix_symmetrize_ensemble", "slod_lod_matrix_combine_ensemble",
         "slod_lod_factor_create_ensemble", "slod_lod_factor_get_info_member", "slod_lod_factor_solve_ensemble",
         "slod_lod_theta_steps_ensemble_direct")
WRAPPERS = ("lod_mass_matrix_ensemble", "lod_matrix_symmetrize_ensemble", "lod_matrix_combine_ensemble",
            "lod_factor_ensemble", "lod_theta_steps_ensemble_direct")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_ensemble_direct_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in WRAPPERS:
        assert callable(getattr(slod_amd.Slod, m))
    for m in ("member_info", "solve", "close"):
        assert callable(getattr(slod_amd.EnsembleFactor, m))


def _refused(g, name, ok, cases):
    """Every (position, bad value) alone makes the call return SLOD_ERR_ARGUMENT and leaves the call's name in the
    handle's error text (a NULL handle or factor leaves it in the thread's)."""
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == -1, (name, at, bad)
        assert name in g.lib.slod_last_error(None if at == 0 else g.h).decode(), (name, at, bad)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_ensemble_direct_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    K, NP = 3, g.num_patches
    stride = 4096                                  # any slab stride: nothing is dereferenced
    slab = NP * stride
    ne2 = g.NE * g.NE
    bad = (C.c_int32 * K)()
    out = C.c_void_p()
    # slod_lod_mass_matrix_ensemble(h, basis, stride, member_stride, n_members, rho, ld_rho, values, ld_m, cols, stream)
    _refused(g, "slod_lod_mass_matrix_ensemble", [g.h, FAKE, stride, slab, K, None, 0, FAKE, K, FAKE, None],
             ((0, None), (1, None), (7, None), (9, None),                 # NULL handle or array (rho may be NULL)
              (4, 0), (4, -1), (4, 65536),                                # n_members
              (8, K - 1),                                                 # ld_m < n_members
              (3, slab - 1), (3, 0)))                                     # member_stride shorter than a slab
    _refused(g, "slod_lod_mass_matrix_ensemble", [g.h, FAKE, stride, slab, K, FAKE, 0, FAKE, K, FAKE, None],
             ((6, ne2 - 1), (6, 1)))                                      # ld_rho non-zero but shorter than a density
    # slod_lod_matrix_symmetrize_ensemble(h, values, ld_in, cols, n_members, out, ld_out, stream)
    _refused(g, "slod_lod_matrix_symmetrize_ensemble", [g.h, FAKE, K, FAKE, K, 2 * FAKE, K, None],
             ((0, None), (1, None), (3, None), (5, None),
              (4, 0), (4, -1), (4, 65536),
              (2, K - 1), (6, K - 1),                                     # ld_in, ld_out
              (5, FAKE)))                                                 # d_out == d_values
    # slod_lod_matrix_combine_ensemble(h, alpha, a, ld_a, beta, b, ld_b, n_members, out, ld_out, stream)
    _refused(g, "slod_lod_matrix_combine_ensemble", [g.h, 1.0, FAKE, K, 0.5, 2 * FAKE, K, K, 3 * FAKE, K, None],
             ((0, None), (2, None), (5, None), (8, None),
              (7, 0), (7, -1), (7, 65536),
              (3, K - 1), (6, K - 1), (9, K - 1)))                        # ld_a, ld_b, ld_out
    # in place with another leading dimension
    assert g.lib.slod_lod_matrix_combine_ensemble(g.h, 1.0, FAKE, K, 0.5, 2 * FAKE, K, K, FAKE, K + 1, None) == -1
    assert "slod_lod_matrix_combine_ensemble" in g.lib.slod_last_error(g.h).decode()
    assert g.lib.slod_lod_matrix_combine_ensemble(g.h, 1.0, FAKE, K, 0.5, 2 * FAKE, K + 1, K, 2 * FAKE, K, None) == -1
    # slod_lod_factor_create_ensemble(h, values, ld_m, n_members, cols, bad_pivot, out)
    _refused(g, "slod_lod_factor_create_ensemble", [g.h, FAKE, K, K, FAKE, bad, C.byref(out)],
             ((0, None), (1, None), (4, None), (6, None),
              (3, 0), (3, -1), (3, 65536),
              (2, K - 1)))                                                # ld_m
    assert out.value is None
    # slod_lod_factor_get_info_member / slod_lod_factor_solve_ensemble: a NULL factor
    info = slod_amd.FactorInfo()
    assert g.lib.slod_lod_factor_get_info_member(None, 0, C.byref(info)) == -1
    assert "slod_lod_factor_get_info_member" in g.lib.slod_last_error(None).decode()
    assert g.lib.slod_lod_factor_solve_ensemble(None, 0, K, FAKE, K, 1, FAKE, K, None) == -1
    assert "slod_lod_factor_solve_ensemble" in g.lib.slod_last_error(None).decode()
    # slod_lod_theta_steps_ensemble_direct(h, f_S, stiffness, ld_m, cols, dt, theta, n_steps, n_members, u, ld_u, load,
    #                                      ld_load, load_step_stride): the factor is checked last
    _refused(g, "slod_lod_theta_steps_ensemble_direct", [g.h, None, FAKE, K, FAKE, 0.01, 1.0, 1, K, FAKE, K, FAKE, K, 0],
             ((0, None), (2, None), (4, None), (9, None),
              (5, 0.0), (5, -0.01), (5, float("nan")),                    # dt
              (6, -0.1), (6, 1.1), (6, float("nan")),                     # theta
              (7, 0), (8, 0), (8, -1), (8, 65536),                        # n_steps, n_members
              (3, K - 1), (10, K - 1), (12, K - 1)))                      # ld_m, ld_u, ld_load
    # with everything else in order, the NULL factor is what is refused
    assert g.lib.slod_lod_theta_steps_ensemble_direct(g.h, None, FAKE, K, FAKE, 0.01, 1.0, 1, K, FAKE, K, None, 0, 0) == -1
    assert "slod_lod_theta_steps_ensemble_direct: NULL factor" in g.lib.slod_last_error(g.h).decode()
    # and through the wrappers
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_mass_matrix_ensemble(FAKE, stride, K, FAKE, FAKE, ld_m=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_symmetrize_ensemble(FAKE, FAKE, K, FAKE)
    assert e.value.code == -1 and "in place" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_combine_ensemble(1.0, FAKE, 1.0, FAKE, 0, FAKE)
    assert e.value.code == -1 and "n_members" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor_ensemble(FAKE, FAKE, K, ld_m=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value) and (e.value.bad_pivot == -1).all()
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_theta_steps_ensemble_direct(None, FAKE, FAKE, 0.01, 2.0, 1, K, FAKE)
    assert e.value.code == -1 and "theta" in str(e.value)


def test_lod_ensemble_direct_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, n_problems=2)
    K, stride = 2, 4096
    calls = (lambda: g.lod_mass_matrix_ensemble(FAKE, stride, K, FAKE, FAKE),
             lambda: g.lod_matrix_symmetrize_ensemble(FAKE, FAKE, K, 2 * FAKE),
             lambda: g.lod_matrix_combine_ensemble(1.0, FAKE, 0.5, FAKE, K, FAKE),
             lambda: g.lod_factor_ensemble(FAKE, FAKE, K))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
