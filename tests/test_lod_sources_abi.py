"""CPU-side checks of the sources on the LOD space (slod_lod_sources_*, slod_lod_inject_*, slod_lod_time_source_arm), after
the pattern of test_lod_receivers_abi.py: the calls are exported, declared with the signatures of include/slod.h and
wrapped; the ABI is still 5; every SLOD_ERR_ARGUMENT that needs no device and no object is returned with the call's name
in slod_last_error; a source is armed and disarmed on a handle.  A sources object cannot exist without a device, so the
refusals that need one are in test_gpu_lod_sources.py and test_gpu_lod_sources_time.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first

SIGNATURES = {
    "slod_lod_sources_create": "slod_handle* slod_lod_receivers* slod_lod_sources**",
    "slod_lod_sources_get_info": "slod_lod_sources* slod_lod_sources_info*",
    "slod_lod_inject_multi": "slod_handle* slod_lod_sources* double* size_t int double* size_t double* size_t void*",
    "slod_lod_inject_ensemble": "slod_handle* slod_lod_sources* int int double* size_t double* size_t double* size_t void*",
    "slod_lod_time_source_arm": "slod_handle* slod_lod_time_source*",
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


def _struct_fields(name):
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s;" % name, _header())
    out = []
    for line in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        out += [w.strip().lstrip("*") for w in line.split(",") if w.strip()]
    return [w.split()[-1].lstrip("*") for w in out]


def test_source_symbols_are_exported_and_declared():
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
    assert hasattr(lib, "slod_lod_sources_destroy") and "slod_lod_sources_destroy" in declared
    assert re.search(r"^void slod_lod_sources_destroy\(slod_lod_sources \*src\);", _header(), re.M)
    assert lib.slod_abi_version() == 5                                     # additions only
    for m in ("lod_sources", "lod_time_source"):
        assert callable(getattr(slod_amd.Slod, m))
    for m in ("inject", "inject_ensemble", "close"):
        assert callable(getattr(slod_amd.Sources, m))
    assert callable(slod_amd.ricker)
    # the structs of the header and their ctypes mirrors, field by field
    assert _struct_fields("slod_lod_time_source") == [f[0] for f in slod_amd.TimeSource._fields_]
    assert _struct_fields("slod_lod_time_source") == ["src", "d_signal", "ld_signal", "sample_stride", "n_samples"]
    assert _struct_fields("slod_lod_sources_info") == [f[0] for f in slod_amd.SourcesInfo._fields_]
    assert _struct_fields("slod_lod_sources_info") == ["n_sources", "n_members", "n_rows_touched", "nnz", "bytes"]


def test_header_documents_the_signal_layout_and_the_sample_convention():
    flat = " ".join(re.sub(r"\n \*", "\n", _header()).split())
    for promised in ("d_signal[j sample_stride + q ld_signal + c]",
                     "takes source and record off the handle as its first action, whatever it returns",
                     "IRK uses sample 2 k + i for stage i of step k (n_samples >= 2 n_steps)",
                     "Newmark uses sample k + 1 for step k",
                     "in ascending e",
                     "Not built: sources in the slod_lod_newmark_accel, harmonic and eigen calls"):
        assert promised in flat, promised


def test_create_and_info_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    lib, name = g.lib, "slod_lod_sources_create"
    out = C.c_void_p()
    assert lib.slod_lod_sources_create(None, FAKE, C.byref(out)) == -1
    assert lib.slod_last_error(None).decode() == name + ": NULL handle"
    assert lib.slod_lod_sources_create(g.h, None, C.byref(out)) == -1
    assert lib.slod_last_error(g.h).decode() == name + ": NULL recv or out"
    assert lib.slod_lod_sources_create(g.h, FAKE, None) == -1
    assert lib.slod_last_error(g.h).decode() == name + ": NULL recv or out"
    assert not out.value
    info = slod_amd.SourcesInfo()
    assert lib.slod_lod_sources_get_info(None, C.byref(info)) == -1
    lib.slod_lod_sources_destroy(None)


def test_inject_argument_checks():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    lib = g.lib
    for name, ok in (("slod_lod_inject_multi", [g.h, None, FAKE, 3, 3, None, 0, FAKE, 3, None]),
                     ("slod_lod_inject_ensemble", [g.h, None, 0, 3, FAKE, 3, None, 0, FAKE, 3, None])):
        assert getattr(lib, name)(*ok) == -1                               # no sources without a device
        assert lib.slod_last_error(g.h).decode() == name + ": NULL sources or array"
        a = list(ok)
        a[0] = None
        assert getattr(lib, name)(*a) == -1
        assert lib.slod_last_error(None).decode() == name + ": NULL handle"


def test_arm_and_disarm():
    slod_amd, g = _handle(nref=2, n_sub=2, oversampling=1, spacedim=1)
    lib = g.lib
    ts = slod_amd.TimeSource(FAKE, FAKE, 1, 1, 4)
    assert lib.slod_lod_time_source_arm(None, C.byref(ts)) == -1
    assert lib.slod_last_error(None).decode() == "slod_lod_time_source_arm: NULL handle"
    assert lib.slod_lod_time_source_arm(g.h, C.byref(ts)) == 0
    assert lib.slod_lod_time_source_arm(g.h, None) == 0                    # disarms
    assert lib.slod_lod_time_source_arm(g.h, None) == 0                    # and again: nothing armed is no error
    ts.src = None
    assert lib.slod_lod_time_source_arm(g.h, C.byref(ts)) == -1
    assert lib.slod_last_error(g.h).decode() == "slod_lod_time_source_arm: NULL src"
    assert g.lod_time_source(None, 0) is None
    # a stepper refused by one of its own checks takes a disarmed handle as it took it before: the message is its own
    assert lib.slod_lod_theta_steps_direct(g.h, None, FAKE, FAKE, 0.1, 1.0, 2, 1, FAKE, 1, None, 0, 0) == -1
    assert lib.slod_last_error(g.h).decode() == "slod_lod_theta_steps_direct: NULL factor"
