"""CPU-side checks of the bilinear form and the Newmark stepper (slod_lod_inner_multi, slod_lod_newmark_accel,
slod_lod_newmark_steps): they are exported and declared, their argument checks come before any device work (so they
answer on a machine without a GPU), and without a GPU the calls fail loudly."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("slod_lod_inner_multi", "slod_lod_newmark_accel", "slod_lod_newmark_steps")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NAN = float("nan")


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_wave_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in ("lod_inner", "lod_newmark_accel", "lod_newmark_steps"):
        assert callable(getattr(slod_amd.Slod, m))


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_wave_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim)
    lib = g.lib
    K, steps = 3, 4
    out = (C.c_double * K)()
    its = (C.c_int * max(K, steps))()
    res = (C.c_double * max(K, steps))()
    kin = (C.c_double * ((steps + 1) * K))()
    pot = (C.c_double * ((steps + 1) * K))()
    # slod_lod_inner_multi(h, values, cols, x, ld_x, y, ld_y, n_rhs, out, stream)
    ok = [g.h, FAKE, FAKE, FAKE, K, FAKE, K, K, out, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (8, None),   # NULL handle or array
                    (7, 0), (7, -1),                                                    # n_rhs < 1
                    (4, K - 1), (6, K - 1)):                                            # ld_x, ld_y < n_rhs
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_inner_multi(*a) == -1, (at, bad)
    assert "slod_lod_inner_multi" in lib.slod_last_error(g.h).decode()
    # slod_lod_newmark_accel(h, stiffness, mass, cols, damp_mass, damp_stiff, n_rhs, u, ld_u, v, ld_v, load, ld_load,
    #                        a, ld_a, tol, maxit, iterations, residual)
    ok = [g.h, FAKE, FAKE, FAKE, 0.1, 0.01, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 1e-12, 10, its, res]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (7, None), (9, None), (13, None),
                    (4, -0.1), (4, NAN), (5, -0.1), (5, NAN),                           # damping
                    (6, 0), (6, -1),                                                    # n_rhs < 1
                    (8, K - 1), (10, K - 1), (12, K - 1), (14, K - 1),                  # ld_u, ld_v, ld_load, ld_a
                    (16, -1)):                                                          # max_iterations < 0
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_newmark_accel(*a) == -1, (at, bad)
    assert "slod_lod_newmark_accel" in lib.slod_last_error(g.h).decode()
    # slod_lod_newmark_steps(h, stiffness, mass, cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_rhs,
    #                        u, ld_u, v, ld_v, a, ld_a, load, ld_load, stride, tol, maxit, iterations, residual,
    #                        kinetic, potential)
    ok = [g.h, FAKE, FAKE, FAKE, 0.01, 0.25, 0.5, 0.1, 0.01, steps, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 0, 1e-12, 10,
          its, res, kin, pot]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (11, None), (13, None), (15, None),
                    (4, 0.0), (4, -0.01), (4, NAN),                                     # dt <= 0
                    (5, -0.01), (5, 0.51), (5, NAN),                                    # beta outside [0, 1/2]
                    (6, -0.01), (6, 1.01), (6, NAN),                                    # gamma outside [0, 1]
                    (7, -0.1), (7, NAN), (8, -0.1), (8, NAN),                           # damping
                    (9, 0), (9, -1),                                                    # n_steps < 1
                    (10, 0), (10, -1),                                                  # n_rhs < 1
                    (12, K - 1), (14, K - 1), (16, K - 1), (18, K - 1),                 # ld_u, ld_v, ld_a, ld_load
                    (21, -1),                                                           # max_iterations < 0
                    (24, None), (25, None)):                                            # one energy array only
        a = list(ok)
        a[at] = bad
        assert lib.slod_lod_newmark_steps(*a) == -1, (at, bad)
    assert "slod_lod_newmark_steps" in lib.slod_last_error(g.h).decode()
    # and through the wrappers
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_inner(FAKE, FAKE, FAKE, FAKE, n_rhs=K, ld_x=K - 1)
    assert e.value.code == -1 and "leading dimension" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_accel(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, damp_mass=-1.0)
    assert e.value.code == -1 and "damping" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_newmark_steps(FAKE, FAKE, FAKE, 0.01, 1, FAKE, FAKE, FAKE, beta=0.75)
    assert e.value.code == -1 and "beta" in str(e.value)


def test_lod_wave_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    calls = (lambda: g.lod_inner(FAKE, FAKE, FAKE, FAKE, n_rhs=2),
             lambda: g.lod_newmark_accel(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, n_rhs=2),
             lambda: g.lod_newmark_steps(FAKE, FAKE, FAKE, 0.01, 2, FAKE, FAKE, FAKE, n_rhs=2),
             lambda: g.lod_newmark_steps(FAKE, FAKE, FAKE, 0.01, 2, FAKE, FAKE, FAKE, beta=0.0, d_load=FAKE,
                                         load_step_stride=64, damp_mass=0.1, energies=False))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
