"""CPU-side checks of the direct solver on the LOD space (slod_lod_factor_create / _get_info / _solve / _destroy) and
the time loops on a factor (slod_lod_theta_steps_direct, slod_lod_newmark_accel_direct, slod_lod_newmark_steps_direct):
they are exported and declared, their argument checks come before any device work (so they answer on a machine without
a GPU), and without a GPU slod_lod_factor_create fails loudly and leaves *out NULL.  A factor cannot exist without a
GPU: the steppers look at the factor after every other argument, so a FAKE factor stands behind each of those checks;
"factor of another handle / row count" and the checks of slod_lod_factor_solve need a factor and are in
test_gpu_lod_factor.py."""
import ctypes as C

import pytest

NAMES = ("slod_lod_factor_create", "slod_lod_factor_get_info", "slod_lod_factor_solve", "slod_lod_factor_destroy",
         "slod_lod_theta_steps_direct", "slod_lod_newmark_accel_direct", "slod_lod_newmark_steps_direct")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NAN = float("nan")


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_factor_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in ("lod_factor", "lod_theta_steps_direct", "lod_newmark_accel_direct", "lod_newmark_steps_direct"):
        assert callable(getattr(slod_amd.Slod, m))
    for m in ("solve", "close"):
        assert callable(getattr(slod_amd.Factor, m))


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_factor_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim)
    lib = g.lib
    err = lambda: lib.slod_last_error(g.h).decode()
    # slod_lod_factor_create(h, values, cols, out)
    out = C.c_void_p(FAKE)
    assert lib.slod_lod_factor_create(None, FAKE, FAKE, C.byref(out)) == -1 and out.value is None
    for at in (1, 2, 3):
        out = C.c_void_p(FAKE)
        a = [g.h, FAKE, FAKE, C.byref(out)]
        a[at] = None
        assert lib.slod_lod_factor_create(*a) == -1, at
        assert "slod_lod_factor_create" in err()
        assert at == 3 or out.value is None
    # slod_lod_factor_get_info / _solve / _destroy on a NULL factor
    info = slod_amd.FactorInfo()
    assert lib.slod_lod_factor_get_info(None, C.byref(info)) == -1
    assert lib.slod_lod_factor_solve(None, FAKE, 1, 1, FAKE, 1, None) == -1
    lib.slod_lod_factor_destroy(None)
    K, steps = 3, 4
    kin = (C.c_double * ((steps + 1) * K))()
    pot = (C.c_double * ((steps + 1) * K))()
    # The factor is looked at last (only that check reads it): a FAKE factor stands behind every other check, and with
    # every other argument in order a NULL factor is named.
    # slod_lod_theta_steps_direct(h, f, stiffness, cols, dt, theta, n_steps, n_rhs, u, ld_u, load, ld_load, stride)
    theta = ([g.h, FAKE, FAKE, FAKE, 0.01, 0.5, steps, K, FAKE, K, FAKE, K, 0],
             ((0, None), (2, None), (3, None), (8, None),                               # NULL handle or array
              (4, 0.0), (4, -0.01), (4, NAN), (5, -0.01), (5, 1.01), (5, NAN),          # dt <= 0, theta outside [0, 1]
              (6, 0), (6, -1), (7, 0), (7, -1),                                         # n_steps < 1, n_rhs < 1
              (9, K - 1), (11, K - 1)))                                                 # ld_u, ld_load
    # slod_lod_newmark_accel_direct(h, f, stiffness, mass, cols, damp_mass, damp_stiff, n_rhs, u, ld_u, v, ld_v, load,
    #                               ld_load, a, ld_a)
    accel = ([g.h, FAKE, FAKE, FAKE, FAKE, 0.1, 0.01, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K],
             ((0, None), (2, None), (3, None), (4, None), (8, None), (10, None), (14, None),
              (5, -0.1), (5, NAN), (6, -0.1), (6, NAN),                                 # damping
              (7, 0), (7, -1),                                                          # n_rhs < 1
              (9, K - 1), (11, K - 1), (13, K - 1), (15, K - 1)))                       # ld_u, ld_v, ld_load, ld_a
    # slod_lod_newmark_steps_direct(h, f, stiffness, mass, cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_rhs,
    #                               u, ld_u, v, ld_v, a, ld_a, load, ld_load, stride, kinetic, potential)
    steps_ = ([g.h, FAKE, FAKE, FAKE, FAKE, 0.01, 0.25, 0.5, 0.1, 0.01, steps, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 0, kin, pot],
              ((0, None), (2, None), (3, None), (4, None), (12, None), (14, None), (16, None),
               (5, 0.0), (5, -0.01), (5, NAN),                                          # dt <= 0
               (6, -0.01), (6, 0.51), (6, NAN),                                         # beta outside [0, 1/2]
               (7, -0.01), (7, 1.01), (7, NAN),                                         # gamma outside [0, 1]
               (8, -0.1), (8, NAN), (9, -0.1), (9, NAN),                                # damping
               (10, 0), (10, -1), (11, 0), (11, -1),                                    # n_steps < 1, n_rhs < 1
               (13, K - 1), (15, K - 1), (17, K - 1), (19, K - 1),                      # ld_u, ld_v, ld_a, ld_load
               (21, None), (22, None)))                                                 # one energy array only
    for name, (ok, bads) in (("slod_lod_theta_steps_direct", theta), ("slod_lod_newmark_accel_direct", accel),
                             ("slod_lod_newmark_steps_direct", steps_)):
        fn = getattr(lib, name)
        for at, bad in bads:
            a = list(ok)
            a[at] = bad
            assert fn(*a) == -1, (name, at, bad)
            assert at == 0 or name + ":" in err(), (name, at, bad, err())
        a = list(ok)
        a[1] = None
        assert fn(*a) == -1
        assert name + ": NULL factor" in err()
    # through the wrappers
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_theta_steps_direct(None, FAKE, FAKE, 0.01, 0.5, 1, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_accel_direct(None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_steps_direct(None, FAKE, FAKE, FAKE, 0.01, 1, FAKE, FAKE, FAKE)
    assert e.value.code == -1 and "NULL factor" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor(None, FAKE)
    assert e.value.code == -1 and "slod_lod_factor_create" in str(e.value)


def test_lod_factor_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device, *out NULL."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    out = C.c_void_p(FAKE)
    assert g.lib.slod_lod_factor_create(g.h, FAKE, FAKE, C.byref(out)) == -3
    assert out.value is None
    assert "no CPU fallback" in g.lib.slod_last_error(g.h).decode()
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_factor(FAKE, FAKE)
    assert e.value.code == -3 and "no CPU fallback" in str(e.value)
