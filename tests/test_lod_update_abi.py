"""CPU-side checks of the refresh block (slod_update_coefficient, slod_dirty_patches, slod_plan_create_dirty,
slod_lod_matrix_update, slod_lod_mass_matrix_update): the calls are exported, declared and wrapped, their status checks
come in the documented order before any device work (so they answer on a machine without a GPU) and name the call, and
without a GPU the calls fail loudly."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("slod_update_coefficient", "slod_dirty_patches", "slod_plan_create_dirty", "slod_lod_matrix_update",
         "slod_lod_mass_matrix_update")
WRAPPERS = ("update_coefficient", "update_coefficient_device", "dirty_patches", "plan_dirty", "lod_matrix_update",
            "lod_mass_matrix_update")
FAKE = 1 << 20   # never dereferenced: the checks reject the call first


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def test_lod_update_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n in NAMES:
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
    assert lib.slod_abi_version() == 5
    for m in WRAPPERS:
        assert callable(getattr(slod_amd.Slod, m))


def _refused(g, name, ok, cases, status=-1):
    """Every (position, bad value) alone makes the call return `status` and leaves the call's name in the handle's
    error text (a NULL handle leaves it in the thread's)."""
    f = getattr(g.lib, name)
    for at, bad in cases:
        a = list(ok)
        a[at] = bad
        assert f(*a) == status, (name, at, bad)
        assert name in g.lib.slod_last_error(None if at == 0 else g.h).decode(), (name, at, bad)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_lod_update_argument_checks(spacedim):
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=2)
    ne = g.NE * g.NE
    data = np.ones(4 * ne)
    ptr = data.ctypes.data
    out = C.c_void_p()
    ids = (C.c_uint32 * g.num_patches)()
    # slod_update_coefficient(h, problem, field, data, layout, count, on_device, d_dirty): the checks of
    # slod_set_coefficient and a NULL dirty array
    _refused(g, "slod_update_coefficient", [g.h, 0, 0, ptr, 1, 4 * ne, 0, FAKE],
             ((0, None), (3, None), (7, None),
              (1, 2), (2, -1), (2, spacedim),                       # problem, field out of range
              (4, 2), (4, -1), (5, ne), (5, 4 * ne + 1)))           # layout, count for the layout
    _refused(g, "slod_update_coefficient", [g.h, 1, spacedim - 1, ptr, 0, ne, 0, FAKE], ((5, 4 * ne), (5, 0)))
    # slod_dirty_patches(h, d_dirty, patches, capacity)
    _refused(g, "slod_dirty_patches", [g.h, FAKE, ids, g.num_patches], ((0, None), (1, None)))
    # slod_plan_create_dirty(h, problem, d_dirty, out)
    _refused(g, "slod_plan_create_dirty", [g.h, 0, FAKE, C.byref(out)], ((0, None), (2, None), (3, None), (1, 2)))
    assert not out.value
    # slod_lod_matrix_update(h, d_dirty, basis, premult, stride, values, ld_m, stream)
    _refused(g, "slod_lod_matrix_update", [g.h, FAKE, FAKE, FAKE, 4096, FAKE, 1, None],
             ((0, None), (1, None), (2, None), (3, None), (5, None), (6, 0)))
    # slod_lod_mass_matrix_update(h, d_dirty, basis, stride, rho, values, stream); rho may be NULL
    _refused(g, "slod_lod_mass_matrix_update", [g.h, FAKE, FAKE, 4096, None, FAKE, None],
             ((0, None), (1, None), (2, None), (5, None)))
    # and through the wrappers
    with pytest.raises(slod_amd.SlodError) as e:
        g.update_coefficient(0, data[:ne], FAKE)                    # per_qp with the count of layout 0
    assert e.value.code == -1 and "slod_update_coefficient" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_update(FAKE, FAKE, FAKE, 4096, FAKE, ld_m=0)
    assert e.value.code == -1 and "ld_m" in str(e.value)


def test_update_coefficient_status_order():
    """ARGUMENT, then UNSUPPORTED (constant_coefficients), then STATE (never set), then DEVICE: a fresh handle answers
    -4 on every machine, and a handle with the reuse quirk -2 even for a field that was never set."""
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    ne = g.NE * g.NE
    data = np.ones(4 * ne)
    f = g.lib.slod_update_coefficient
    assert f(g.h, 0, 0, data.ctypes.data, 1, 4 * ne, 0, FAKE) == -4
    assert "slod_update_coefficient" in g.lib.slod_last_error(g.h).decode()
    assert f(g.h, 0, 0, data.ctypes.data, 1, 4 * ne, 0, None) == -1           # the argument check comes first
    with pytest.raises(slod_amd.SlodError) as e:
        g.update_coefficient(0, data, FAKE)
    assert e.value.code == -4 and "not set" in str(e.value)
    _, q1 = _handle(nref=3, n_sub=2, oversampling=1, reuse_full=1)
    ne = q1.NE * q1.NE
    data = np.ones(4 * ne)
    assert f(q1.h, 0, 0, data.ctypes.data, 1, 4 * ne, 0, FAKE) == -2
    assert "slod_update_coefficient" in q1.lib.slod_last_error(q1.h).decode()
    assert "constant_coefficients" in q1.lib.slod_last_error(q1.h).decode()
    assert f(q1.h, 0, 1, data.ctypes.data, 1, 4 * ne, 0, FAKE) == -1          # field out of range: still the first check


def test_lod_update_without_gpu_fails_loudly():
    """No CPU fallback, as test_compute_without_gpu_fails_loudly: SLOD_ERR_DEVICE without a HIP device.
    (slod_update_coefficient cannot get there: without a device no field was ever set, and that is -4.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    calls = (lambda: g.dirty_patches(FAKE),
             lambda: g.dirty_patches(FAKE, count_only=True),
             lambda: g.plan_dirty(FAKE),
             lambda: g.lod_matrix_update(FAKE, FAKE, FAKE, 4096, FAKE),
             lambda: g.lod_mass_matrix_update(FAKE, FAKE, 4096, FAKE))
    for call in calls:
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -3
        assert "no CPU fallback" in str(e.value)
