"""CPU-side checks of the coarse FEM(H) entry points (slod_coarse_coefficient, slod_coarse_fem_rhs,
slod_coarse_fem_solve, slod_coarse_interpolate): they are exported and declared, their argument checks come
before any device work (so they answer on a machine without a GPU), and without a GPU the calls fail loudly.
The SLOD_ERR_STATE answer ("coefficient not set") comes after the handle has got its device, as in
slod_compute_error_norms, so it is checked on the GPU (tests/test_gpu_coarse_fem.py)."""
import ctypes as C

import pytest

NAMES = ("slod_coarse_coefficient", "slod_coarse_fem_rhs", "slod_coarse_fem_solve", "slod_coarse_interpolate")
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_coarse_fem_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in ("coarse_coefficient", "coarse_fem_rhs", "coarse_fem_solve", "coarse_interpolate"):
        assert callable(getattr(slod_amd.Slod, m))


@pytest.mark.parametrize("spacedim", [1, 2])
def test_coarse_fem_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim)
    lib, res = g.lib, C.c_double()
    # slod_coarse_coefficient: NULL handle, NULL out, problem and field out of range
    assert lib.slod_coarse_coefficient(None, 0, 0, FAKE, None) == -1
    assert lib.slod_coarse_coefficient(g.h, 0, 0, None, None) == -1
    assert lib.slod_coarse_coefficient(g.h, 1, 0, FAKE, None) == -1
    assert "slod_coarse_coefficient" in lib.slod_last_error(g.h).decode()
    assert "out of range" in lib.slod_last_error(g.h).decode()
    assert lib.slod_coarse_coefficient(g.h, 0, spacedim, FAKE, None) == -1
    assert lib.slod_coarse_coefficient(g.h, 0, -1, FAKE, None) == -1
    assert "out of range" in lib.slod_last_error(g.h).decode()
    # slod_coarse_fem_rhs: NULL handle, NULL output (a NULL f means f = 1)
    assert lib.slod_coarse_fem_rhs(None, None, FAKE, None) == -1
    assert lib.slod_coarse_fem_rhs(g.h, None, None, None) == -1
    assert lib.slod_coarse_fem_rhs(g.h, FAKE, None, None) == -1
    # slod_coarse_fem_solve: NULL handle / rhs / solution, negative iteration limit, problem out of range
    assert lib.slod_coarse_fem_solve(None, 0, FAKE, FAKE, 1e-12, 10, C.byref(res)) == -1
    assert lib.slod_coarse_fem_solve(g.h, 0, None, FAKE, 1e-12, 10, C.byref(res)) == -1
    assert lib.slod_coarse_fem_solve(g.h, 0, FAKE, None, 1e-12, 10, C.byref(res)) == -1
    assert lib.slod_coarse_fem_solve(g.h, 0, FAKE, FAKE, 1e-12, -1, C.byref(res)) == -1
    assert lib.slod_coarse_fem_solve(g.h, 1, FAKE, FAKE, 1e-12, 10, C.byref(res)) == -1
    assert "slod_coarse_fem_solve: problem out of range" in lib.slod_last_error(g.h).decode()
    # slod_coarse_interpolate: NULL handle / input / output
    assert lib.slod_coarse_interpolate(None, FAKE, FAKE, None) == -1
    assert lib.slod_coarse_interpolate(g.h, None, FAKE, None) == -1
    assert lib.slod_coarse_interpolate(g.h, FAKE, None, None) == -1
    # and through the wrapper
    with pytest.raises(slod_amd.SlodError) as e:
        g.coarse_coefficient(spacedim, FAKE)
    assert e.value.code == -1
    with pytest.raises(slod_amd.SlodError) as e:
        g.coarse_fem_solve(FAKE, FAKE, problem=3)
    assert e.value.code == -1 and "problem out of range" in str(e.value)


def test_coarse_fem_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    calls = (lambda: g.coarse_coefficient(0, FAKE), lambda: g.coarse_fem_rhs(None, FAKE),
             lambda: g.coarse_fem_solve(FAKE, FAKE), lambda: g.coarse_interpolate(FAKE, FAKE))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
