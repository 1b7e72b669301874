"""CPU-side checks of the receivers on the LOD space (slod_lod_receivers_*, slod_lod_observe_*, slod_lod_time_record_arm),
after the pattern of test_lod_irk_abi.py: the calls are exported, declared with the signatures of include/slod.h and
wrapped; every SLOD_ERR_ARGUMENT that needs no device is returned before any device work (so on a machine without a GPU)
with the call's name in slod_last_error; a valid slod_lod_receivers_create is SLOD_ERR_DEVICE without a GPU; a record is
armed and disarmed on a handle.  A receivers object cannot exist without a device, so the refusals that need one are in
test_gpu_lod_receivers.py and test_gpu_lod_receivers_time.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NANF, INF = float("nan"), float("inf")

SIGNATURES = {
    "slod_lod_receiver_capacity": "slod_handle*",
    "slod_lod_receiver_pattern": "slod_handle* uint32_t uint32_t* size_t",
    "slod_lod_receivers_create": "slod_handle* int uint32_t* uint32_t* int32_t* double* double* size_t size_t int "
                                 "slod_lod_receivers**",
    "slod_lod_receivers_get_info": "slod_lod_receivers* slod_lod_receivers_info*",
    "slod_lod_receivers_rows": "slod_lod_receivers* int uint32_t* uint32_t* double*",
    "slod_lod_observe_multi": "slod_handle* slod_lod_receivers* double* size_t int double* size_t void*",
    "slod_lod_observe_ensemble": "slod_handle* slod_lod_receivers* int int double* size_t double* size_t void*",
    "slod_lod_time_record_arm": "slod_handle* slod_lod_time_record*",
}
SCALARS = {"double": C.c_double, "int": C.c_int, "size_t": C.c_size_t, "uint32_t": C.c_uint32}


def _handle(**kw):
    import slod_amd
    return slod_amd, slod_amd.Slod(**kw)


def _header():
    return open(os.path.join(ROOT, "include", "slod.h")).read()


def _declared_types(name):
    m = re.search(r"^int %s\((.*?)\);" % name, _header(), re.M | re.S)
    assert m, "not declared: " + name
    out = []
    for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        p = p.replace("const", " ").strip()
        stars = p.count("*")
        words = p.replace("*", " ").split()
        out.append(" ".join(words[:-1]) + "*" * stars)
    return out


def test_receiver_symbols_are_exported_and_declared():
    import slod_amd
    lib = slod_amd.load()
    declared = slod_amd.declared_symbols()
    for n, sig in SIGNATURES.items():
        assert hasattr(lib, n), "missing export " + n
        assert n in declared, "not declared in include/slod.h: " + n
        want = sig.split()
        assert _declared_types(n) == want, (n, _declared_types(n))
        got = getattr(lib, n).argtypes
        assert len(got) == len(want), n
        for t, w in zip(got, want):
            if w.endswith("*"):
                assert t is C.c_void_p or issubclass(t, C._Pointer), (n, w, t)
            else:
                assert t is SCALARS[w], (n, w, t)
    assert hasattr(lib, "slod_lod_receivers_destroy") and "slod_lod_receivers_destroy" in declared
    assert re.search(r"^void slod_lod_receivers_destroy\(slod_lod_receivers \*recv\);", _header(), re.M)
    assert lib.slod_abi_version() == 5
    for m in ("lod_receivers", "lod_receiver_pattern", "lod_receiver_capacity", "lod_time_record"):
        assert callable(getattr(slod_amd.Slod, m))
    for m in ("rows", "observe", "observe_ensemble", "close"):
        assert callable(getattr(slod_amd.Receivers, m))
    assert callable(slod_amd.point_terms)
    assert (slod_amd.RECORD_U, slod_amd.RECORD_V) == (1, 2)
    assert re.search(r"SLOD_RECORD_U\s*=\s*1\s*,\s*SLOD_RECORD_V\s*=\s*2", _header())
    # the record struct of the header and its ctypes mirror, field by field
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*slod_lod_time_record;", _header())
    fields = [re.sub(r"/\*.*?\*/", "", l).strip().rstrip(";").split()[-1].lstrip("*") for l in m.group(1).strip().splitlines()]
    assert fields == [f[0] for f in slod_amd.TimeRecord._fields_]
    assert fields == ["recv", "what", "every", "d_trace", "ld_trace", "record_stride", "capacity"]


def test_header_documents_the_trace_layout_and_the_one_shot_rule():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())
    for promised in ("d_trace[j record_stride + (w n_recv + q) ld_trace + c]",
                     "takes the record off the handle as its first action and is the only call that sees it, whatever it returns",
                     "record 0 the entry state",
                     "capacity < n_steps / every + 1",
                     "values[e K + m]",
                     "Not built: time signals that scale a load inside the loop (sources)"):
        assert promised in flat, promised


def _create_args(g, n_recv=2, begin=(0, 1, 3), node=(0, 5, 6), comp=(0, 0, 0), weight=(1.0, 0.5, -0.5), basis=FAKE, stride=None,
                 mstride=0, K=1):
    u32p = C.POINTER(C.c_uint32)
    a = [np.array(begin, dtype=np.uint32), np.array(node, dtype=np.uint32), np.array(comp, dtype=np.int32),
         np.array(weight, dtype=np.float64)]
    full = g.spacedim ** 2 * (g.cfg.n_subdivisions * (2 * g.cfg.oversampling + 1) + 1) ** 2
    out = C.c_void_p()
    args = [g.h, n_recv, a[0].ctypes.data_as(u32p), a[1].ctypes.data_as(u32p), a[2].ctypes.data_as(C.POINTER(C.c_int32)),
            a[3].ctypes.data_as(C.POINTER(C.c_double)), basis, full if stride is None else stride, mstride, K, C.byref(out)]
    return args, a, out


def test_receivers_create_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    name = "slod_lod_receivers_create"
    f = g.lib.slod_lod_receivers_create
    n_node = (g.NE + 1) ** 2

    def refused(word, at=None, bad=None, **kw):
        args, keep, out = _create_args(g, **kw)
        if at is not None:
            args[at] = bad
        assert f(*args) == -1, (word, at, kw)
        msg = g.lib.slod_last_error(g.h if at != 0 else None).decode()
        assert msg.startswith(name + ":") and word in msg, (word, at, kw, msg)
        assert not out.value

    for at in (0, 2, 3, 4, 5, 6, 10):
        refused("NULL", at, None)
    refused("n_recv < 1", 1, 0)
    refused("n_recv < 1", 1, -2)
    refused("has no term", begin=(0, 0, 3))
    refused("has no term", begin=(0, 3, 3))
    refused("not monotone", begin=(0, 2, 1))
    refused("not monotone", begin=(1, 2, 3))
    refused("node out of range", node=(0, n_node, 6))
    refused("component out of range", comp=(0, 1, 0))
    refused("component out of range", comp=(0, -1, 0))
    for w in (NANF, INF, -INF):
        refused("weight is not finite", weight=(1.0, w, 1.0))
    refused("n_members < 1 or > 65535", K=0)
    refused("n_members < 1 or > 65535", K=65536)
    full = (2 * 3 + 1) ** 2
    refused("stride below the words of a patch", stride=full - 1)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_receivers([[(n_node, 0, 1.0)]], FAKE, full)
    assert e.value.code == -1 and name + ":" in str(e.value)


def test_nnz_beyond_31_bits_is_refused():
    slod_amd, g = _handle(n_cells=16, n_sub=1, oversampling=16, spacedim=2)   # every patch is the domain: 512 entries a term
    assert g.lod_receiver_capacity() >= len(g.lod_receiver_pattern(0)) == 512
    n_term = (1 << 31) // 512
    begin = np.array([0, n_term], dtype=np.uint32)
    node = np.zeros(n_term, dtype=np.uint32)
    comp = np.zeros(n_term, dtype=np.int32)
    weight = np.ones(n_term)
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_receivers((begin, node, comp, weight), FAKE, 4 * 17 * 17, raw=True)
    assert e.value.code == -1 and "slod_lod_receivers_create: nnz does not fit 31 bits" in str(e.value)


def test_pattern_and_capacity_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=2)
    lib = g.lib
    assert lib.slod_lod_receiver_capacity(None) == -1
    assert lib.slod_lod_receiver_capacity(g.h) == 16 * 2
    buf = (C.c_uint32 * 32)()
    assert lib.slod_lod_receiver_pattern(None, 0, buf, 32) == -1 and lib.slod_lod_receiver_pattern(g.h, 0, None, 32) == -1
    centre = 4 + 4 * 9                                    # the corner shared by the four middle cells of the 4 x 4 grid
    assert lib.slod_lod_receiver_pattern(g.h, centre, buf, 32) == 32
    assert lib.slod_lod_receiver_pattern(g.h, centre, buf, 31) == -1
    assert lib.slod_last_error(g.h).decode() == "slod_lod_receiver_pattern: buffer too small"
    assert lib.slod_lod_receiver_pattern(g.h, 0, buf, 32) == 4 * 2     # the domain corner: cells (0..1) x (0..1)


def test_observe_and_info_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    lib = g.lib
    for name, ok in (("slod_lod_observe_multi", [g.h, None, FAKE, 3, 3, FAKE, 3, None]),
                     ("slod_lod_observe_ensemble", [g.h, None, 0, 3, FAKE, 3, FAKE, 3, None])):
        assert getattr(lib, name)(*ok) == -1                               # no receivers without a device
        assert lib.slod_last_error(g.h).decode().startswith(name + ": NULL")
        a = list(ok)
        a[0] = None
        assert getattr(lib, name)(*a) == -1
        assert lib.slod_last_error(None).decode().startswith(name + ": NULL handle")
    info = slod_amd.ReceiversInfo()
    assert lib.slod_lod_receivers_get_info(None, C.byref(info)) == -1
    assert lib.slod_lod_receivers_rows(None, 0, None, None, None) == -1
    lib.slod_lod_receivers_destroy(None)


def test_arm_and_disarm():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    lib = g.lib
    rec = slod_amd.TimeRecord(FAKE, slod_amd.RECORD_U, 1, FAKE, 1, 1, 4)
    assert lib.slod_lod_time_record_arm(None, C.byref(rec)) == -1
    assert lib.slod_last_error(None).decode() == "slod_lod_time_record_arm: NULL handle"
    assert lib.slod_lod_time_record_arm(g.h, C.byref(rec)) == 0
    assert lib.slod_lod_time_record_arm(g.h, None) == 0                    # disarms
    assert lib.slod_lod_time_record_arm(g.h, None) == 0                    # and again: nothing armed is no error
    rec.recv = None
    assert lib.slod_lod_time_record_arm(g.h, C.byref(rec)) == -1
    assert lib.slod_last_error(g.h).decode() == "slod_lod_time_record_arm: NULL recv"
    assert g.lod_time_record(None, 0) is None
    # a stepper refused by one of its own checks takes a disarmed handle as it took it before: the message is its own
    assert lib.slod_lod_theta_steps_direct(g.h, None, FAKE, FAKE, 0.1, 1.0, 2, 1, FAKE, 1, None, 0, 0) == -1
    assert lib.slod_last_error(g.h).decode() == "slod_lod_theta_steps_direct: NULL factor"


def test_receivers_without_gpu_fail_loudly():
    """No CPU fallback: with valid arguments the create call reaches the device and is SLOD_ERR_DEVICE without one; the
    host-only pattern call answers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1)
    assert len(g.lod_receiver_pattern(0)) == 4
    args, keep, out = _create_args(g)
    assert g.lib.slod_lod_receivers_create(*args) == -3 and not out.value
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_receivers([slod_amd.point_terms(g.NE, 1, 0.3, 0.6)], FAKE, 49)
    assert e.value.code == -3 and "no CPU fallback" in str(e.value)
