"""CPU-side checks of slod_compute_error_norms: it is exported, its argument checks come before any device
work (so they answer on a machine without a GPU), and without a GPU the call fails loudly."""
import ctypes as C

import pytest


def _lib_and_handle(**kw):
    import slod_amd
    g = slod_amd.Slod(**kw)
    return slod_amd, g


def test_error_norms_symbol_is_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    assert hasattr(lib, "slod_compute_error_norms")
    assert "slod_compute_error_norms" in slod_amd.declared_symbols()
    assert C.sizeof(slod_amd.ErrorNorms) == 10 * 8
    assert lib.slod_abi_version() == 5


def test_error_norms_argument_checks():
    slod_amd, g = _lib_and_handle(nref=2, n_sub=2, oversampling=1)
    lib = g.lib
    out = slod_amd.ErrorNorms()
    fake = 1 << 20   # never dereferenced: the argument checks reject the call first
    # NULL handle, NULL out
    assert lib.slod_compute_error_norms(None, 0, None, None, None, None, C.byref(out), None) == -1
    assert lib.slod_compute_error_norms(g.h, 0, None, None, None, None, None, None) == -1
    # exact values without gradients, gradients without values
    assert lib.slod_compute_error_norms(g.h, 0, None, None, fake, None, C.byref(out), None) == -1
    assert lib.slod_compute_error_norms(g.h, 0, None, None, None, fake, C.byref(out), None) == -1
    assert "together" in lib.slod_last_error(g.h).decode()
    # problem out of range, misaligned exact arrays
    assert lib.slod_compute_error_norms(g.h, 1, None, None, None, None, C.byref(out), None) == -1
    assert lib.slod_compute_error_norms(g.h, 0, None, None, fake + 8, fake, C.byref(out), None) == -1
    with pytest.raises(slod_amd.SlodError) as e:
        g.error_norms(None, d_exact=fake)
    assert e.value.code == -1


def test_error_norms_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _lib_and_handle(nref=2, n_sub=2, oversampling=1)
    with pytest.raises(slod_amd.SlodError) as e:
        g.error_norms(None)
    assert e.value.code == -3
