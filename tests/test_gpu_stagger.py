"""k_solve_tw's wave priorities by workgroup class (SLOD_STAGGER, SLOD_STAGGER_ROW; the modes are listed at the top
of slod_dispatch.cpp).  Priorities change no arithmetic: for every mode (phi, psi) must equal SLOD_STAGGER=0 as 64-bit
words, plan.status() must be clean, and mode 0 must hold the oracle bars of test_gpu_parity.py (phi 1e-10, psi
1e-10 * ||A||_inf).  Every plan takes SLOD_STAGGER_ROW=16, so that its 64 patches fall into all four classes.  The
dispatcher's rule (mode 0 for vector plans and for plans larger than one resident set) is read off the launch log.
Host only: the class of every block, from the formula the kernel uses (tools/dump_stagger_class.cpp).  Nothing here
measures time."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_fields
from lod_cases import _bits, _check_patch, _mk, _upload

gpu = pytest.mark.gpu
MODES = (0, 1, 2, 3, 4)
ROW = 16
PLANS = {
    # 64 patches, the interior ones 5 x 5 cells of 8: k_solve_tw<5,1>, the benchmark's instantiation
    "poisson-T5": (dict(nref=3, n_sub=8, oversampling=2), "D1e4", "k_solve_tw<5,1>"),
    # another lane tile: m_max = 19
    "poisson-T3": (dict(nref=3, n_sub=4, oversampling=2), "D1e4", "k_solve_tw<3,1>"),
    # a vector plan: the dispatcher keeps it at mode 0
    "elasticity": (dict(nref=3, n_sub=4, oversampling=2, spacedim=2), "D100", "k_solve_tw<"),
}
_LINE = re.compile(r"^\[slod\] (k_solve_tw<\d+,\d+>): (\d+) patches, lds \d+ B, occupancy \d+ blocks/CU, stagger (\d) row (\d+), "
                   r"backward K split [01], M in the sweeps [01]$")
_runs = {}


def _launches(err):
    """(kernel, patches, mode, row) of every k_solve_tw launch in a SLOD_DEBUG log; every such line must parse."""
    out = []
    for ln in err.splitlines():
        if "k_solve_tw<" in ln:
            m = _LINE.match(ln)
            assert m, "launch log line: %r" % ln
            out.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return out


def _run(so, capfd, monkeypatch, name, mode, extra=None):
    """One plan of all patches under SLOD_STAGGER=mode: (cfg, fields, words of phi, words of psi, stride, launches);
    computed once per (plan, mode, extra knobs), read-only."""
    import torch
    key = (name, mode, tuple(sorted((extra or {}).items())))
    if key not in _runs:
        kw, dist, _ = PLANS[name]
        monkeypatch.setenv("SLOD_DEBUG", "1")
        monkeypatch.setenv("SLOD_STAGGER", str(mode))
        monkeypatch.setenv("SLOD_STAGGER_ROW", str(ROW))
        for k, v in (extra or {}).items():
            monkeypatch.setenv(k, v)
        cfg, g = _mk(so, stabilize=1, **kw)
        fields = make_fields(so, cfg, dist)
        _upload(g, fields)
        ids = np.arange(g.num_patches, dtype=np.uint32)
        assert len(ids) == 64
        capfd.readouterr()
        plan = g.plan(ids)
        dev = torch.device("cuda", 0)
        b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
        q = torch.zeros_like(b)
        plan.execute(b.data_ptr(), q.data_ptr())
        torch.cuda.synchronize()
        plan.status()  # raises unless the execute was clean
        launches = _launches(capfd.readouterr().err)
        hb, hq = _bits(b), _bits(q)
        hb.setflags(write=False)
        hq.setflags(write=False)
        _runs[key] = (cfg, fields, hb, hq, plan.stride, launches)
        plan.close()
    return _runs[key]


def _oracle_bars(so, run, label):
    cfg, fields, hb, hq, stride, _ = run
    basis, premult = hb.view(np.float64), hq.view(np.float64)
    for pid in range(64):
        _check_patch(so, cfg, fields, pid, basis, premult, pid * stride, label)


@gpu
@pytest.mark.parametrize("name", ["poisson-T5", "poisson-T3"])
def test_mode0_holds_the_oracle_bars(so, capfd, monkeypatch, name):
    run = _run(so, capfd, monkeypatch, name, 0)
    assert run[5] == [(PLANS[name][2], 64, 0, ROW)], run[5]
    _oracle_bars(so, run, name + " stagger 0")


@gpu
@pytest.mark.parametrize("mode", MODES[1:])
@pytest.mark.parametrize("name", ["poisson-T5", "poisson-T3"])
def test_every_mode_has_the_bits_of_mode0(so, capfd, monkeypatch, name, mode):
    ref = _run(so, capfd, monkeypatch, name, 0)
    run = _run(so, capfd, monkeypatch, name, mode)
    assert run[5] == [(PLANS[name][2], 64, mode, ROW)], run[5]
    assert np.array_equal(run[2], ref[2]), "%s stagger %d: phi differs from stagger 0" % (name, mode)
    assert np.array_equal(run[3], ref[3]), "%s stagger %d: psi differs from stagger 0" % (name, mode)


@gpu
def test_vector_plans_stay_at_mode0(so, capfd, monkeypatch):
    ref = _run(so, capfd, monkeypatch, "elasticity", 0)
    _oracle_bars(so, ref, "elasticity stagger 0")
    for mode in MODES:
        run = _run(so, capfd, monkeypatch, "elasticity", mode)
        assert run[5] and all(k.startswith("k_solve_tw<") and k.endswith(",2>") and m == 0 and r == ROW
                              for k, _, m, r in run[5]), run[5]
        assert np.array_equal(run[2], ref[2]) and np.array_equal(run[3], ref[3]), "elasticity stagger %d" % mode


@gpu
def test_plans_beyond_one_resident_set_get_mode0(so, capfd, monkeypatch):
    """SLOD_WORKSPACE_MB=1 (the knob of the chunking tests): the 64 patches of the T = 3 plan run in several launches
    that re-use the workspace slots, so its rows are no co-residents: every launch reports mode 0 whatever the knob
    says, and the words are those of the one-launch plan."""
    ref = _run(so, capfd, monkeypatch, "poisson-T3", 0)
    run = _run(so, capfd, monkeypatch, "poisson-T3", 2, {"SLOD_WORKSPACE_MB": "1"})
    assert len(run[5]) >= 2 and sum(n for _, n, _, _ in run[5]) == 64, run[5]
    assert all(m == 0 for _, _, m, _ in run[5]), run[5]
    assert np.array_equal(run[2], ref[2]) and np.array_equal(run[3], ref[3])


@gpu
def test_mode0_log_line_is_the_old_one_plus_the_new_fields(so, capfd, monkeypatch):
    """_LINE is the launch line as it was with ', stagger M row R' after the occupancy (the parsers of the older tests read
    the K split up to its comma and M to the end of the line): _launches() asserts that every line parses."""
    run = _run(so, capfd, monkeypatch, "poisson-T5", 0)
    assert run[5] == [("k_solve_tw<5,1>", 64, 0, ROW)]


def test_class_of_every_block(tmp_path):
    """Host only: tools/dump_stagger_class.cpp prints slod_stagger_class (slod_device.h, what the kernel calls) for the
    blocks of a launch: (b / row) & 3."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "dump_stagger_class")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "dealii-slod_amd", "csrc"),
                           os.path.join(ROOT, "tools", "dump_stagger_class.cpp"), "-o", exe])
    for row in (1, 16, 256):
        for n in (1, row, row + 1, 4 * row, 4 * row + 3):
            out = subprocess.run([exe, str(row), str(n)], capture_output=True, text=True, check=True).stdout.split()
            assert [int(x) for x in out] == [(b // row) & 3 for b in range(n)], (row, n)
    # row = 1, 4 blocks: one block per class, in launch order; a fifth block wraps round
    out = subprocess.run([exe, "1", "5"], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "1", "2", "3", "0"]
