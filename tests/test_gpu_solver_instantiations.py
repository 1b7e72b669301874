"""Every patch-solve template instantiation a plan can reach, launched once and compared with the oracle.

Which of k_solve_tw<T,S>, k_solve_mf<NT,S>, k_solve<R,S,TW> (coop) and k_solve_nd<NV,T> a plan gets is
decided at run time from (S, m_max, nc_max, n_patches) and the SLOD_SOLVE / SLOD_TWISTED knobs
(slod_choose_solver, slod_launch_solve_*).  Each instantiation has its own register tiles, its own padding
of lines narrower than the tile and an LDS carve-up that a host function mirrors: a kernel can be wrong for
one size only.  ROWS is the table of DESIGN.md ("Patch-solve instantiations") as test cases; the launch log
(SLOD_DEBUG=1) proves which instantiation ran, test_rows_cover_every_reachable_instantiation (no GPU) that
no reachable one is missing.

m_max = S * (min(mx, my) * n_sub - 1) over the plan's patches; tw takes T = the smallest of
{2,3,4,5,6,8,10,12,14} with 8 T >= m_max, mf NT = ceil(m_max / 16), coop R = ceil(m_max / 16).

Bars (the project's, flat -- every configuration here has oversampling <= 2 and is well conditioned: the
oracle's spread under 1e-13 solver noise is at most 1.4e-11 on every patch, so.selection_conditioning):
  |dphi| <= 1e-10, |dpsi| <= 1e-10 * ||A||_inf           lod_cases._check_patch
  (n_cut, n_dropped) equal to the oracle's               where the oracle's decisions are stable
  |dX| <= 1e-11 * max|X|                                 test_gpu_parity.test_patch_solution_matches_oracle
"""
import re

import numpy as np
import pytest

from conftest import make_fields
from lod_cases import _check_patch, _decisions, _mk, _upload

TOL_X = 1e-11


def _cfg(n_sub, l=1, nref=2, s=1):
    return dict(nref=nref, n_sub=n_sub, oversampling=l, spacedim=s, stabilize=1)


# patch filters: which patches of the configuration the plan holds
def _all(i):
    return True


def _corners(i):
    """the 2 x 2-cell patches in the corners of the domain (oversampling 1)"""
    return i.mx == 2 and i.my == 2


def _at_most_4_cells_wide(i):
    return min(i.mx, i.my) <= 4


def _row(name, kw, expect, solve=None, twisted=None, filt=_all):
    env = {}
    if solve is not None:
        env["SLOD_SOLVE"] = solve
    if twisted is not None:
        env["SLOD_TWISTED"] = str(twisted)
    return pytest.param(env, kw, filt, expect, id=name)


def _coop(name, kw, r, s, filt=_all, tw1=1):
    """SLOD_SOLVE=coop with SLOD_TWISTED=0 and =1; tw1 = 0: the twisted carve-up exceeds 160 KB of LDS and
    the dispatcher falls back to one chain"""
    return [_row("coop-%s-tw0" % name, kw, "k_solve<%d,%d,0>" % (r, s), "coop", 0, filt),
            _row("coop-%s-tw1" % name, kw, "k_solve<%d,%d,%d>" % (r, s, tw1), "coop", 1, filt)]


ROWS = [
    # ---- tw, vector problems: the automatic production kernel for m_max > 16
    _row("tw-s2-m22", _cfg(4, s=2), "k_solve_tw<3,2>"),
    _row("tw-s2-m28", _cfg(5, s=2), "k_solve_tw<4,2>"),
    _row("tw-s2-m40-exact", _cfg(7, s=2), "k_solve_tw<5,2>"),
    _row("tw-s2-m46", _cfg(8, s=2), "k_solve_tw<6,2>"),
    _row("tw-s2-m48-exact-nc50", _cfg(5, l=2, nref=3, s=2), "k_solve_tw<6,2>"),
    _row("tw-s2-m64-exact", _cfg(11, s=2), "k_solve_tw<8,2>"),
    _row("tw-s2-m66", _cfg(17, s=2), "k_solve_tw<10,2>", filt=_corners),
    _row("tw-s2-m94", _cfg(16, s=2), "k_solve_tw<12,2>"),
    _row("tw-s2-m112-exact", _cfg(19, s=2), "k_solve_tw<14,2>"),
    # ---- tw, scalar problems: the line fills the lane tile exactly (m_max == 8 T)
    _row("tw-s1-m24-exact", _cfg(5, l=2, nref=3), "k_solve_tw<3,1>"),
    _row("tw-s1-m32-exact", _cfg(11), "k_solve_tw<4,1>"),
    _row("tw-s1-m64-exact", _cfg(13, l=2, nref=3), "k_solve_tw<8,1>"),
    _row("tw-s1-m80-exact", _cfg(27), "k_solve_tw<10,1>"),
    # ---- tw, scalar problems: one dof past the previous tile (the most padding a tile ever sees)
    _row("tw-s1-m25", _cfg(13), "k_solve_tw<4,1>", filt=_corners),
    _row("tw-s1-m33", _cfg(17), "k_solve_tw<5,1>", filt=_corners),
    _row("tw-s1-m41", _cfg(14), "k_solve_tw<6,1>"),
    _row("tw-s1-m49", _cfg(10, l=2, nref=3), "k_solve_tw<8,1>"),
    _row("tw-s1-m65", _cfg(22), "k_solve_tw<10,1>"),
    _row("tw-s1-m81", _cfg(41), "k_solve_tw<12,1>", filt=_corners),
    _row("tw-s1-m97", _cfg(49), "k_solve_tw<14,1>", filt=_corners),
    # ---- mf, scalar problems (by knob only)
    _row("mf-s1-m14", _cfg(5), "k_solve_mf<1,1>", "mf"),
    _row("mf-s1-m32", _cfg(11), "k_solve_mf<2,1>", "mf"),
    _row("mf-s1-m47", _cfg(16, nref=3), "k_solve_mf<3,1>", "mf"),
    _row("mf-s1-m64", _cfg(13, l=2, nref=3), "k_solve_mf<4,1>", "mf"),
    _row("mf-s1-m80", _cfg(27), "k_solve_mf<5,1>", "mf"),
    _row("mf-s1-m81", _cfg(41), "k_solve_mf<6,1>", "mf", filt=_corners),
    _row("mf-s1-m110", _cfg(37), "k_solve_mf<7,1>", "mf"),
    # ---- mf, vector problems: the automatic choice up to m_max = 16 (no knob set), by knob beyond
    _row("mf-s2-m10-auto", _cfg(2, s=2), "k_solve_mf<1,2>"),
    _row("mf-s2-m16-auto", _cfg(3, s=2), "k_solve_mf<1,2>"),
    _row("mf-s2-m22", _cfg(4, s=2), "k_solve_mf<2,2>", "mf"),
    _row("mf-s2-m46", _cfg(8, s=2), "k_solve_mf<3,2>", "mf"),
    _row("mf-s2-m64", _cfg(11, s=2), "k_solve_mf<4,2>", "mf"),
    _row("mf-s2-m78", _cfg(20, s=2), "k_solve_mf<5,2>", "mf", filt=_corners),
    # ---- coop (by knob only), one chain and two
    *_coop("s1-m14", _cfg(5), 1, 1),
    *_coop("s1-m32", _cfg(11), 2, 1),
    *_coop("s1-m41", _cfg(14), 3, 1),
    *_coop("s1-m49", _cfg(10, l=2, nref=3), 4, 1),
    *_coop("s1-m65", _cfg(22), 5, 1),
    *_coop("s1-m81", _cfg(41), 6, 1, filt=_corners),
    *_coop("s1-m97", _cfg(49), 7, 1, filt=_corners, tw1=0),
    *_coop("s2-m16", _cfg(3, s=2), 1, 2),
    *_coop("s2-m28", _cfg(5, s=2), 2, 2),
    *_coop("s2-m46", _cfg(8, s=2), 3, 2),
    *_coop("s2-m64", _cfg(11, s=2), 4, 2),
    *_coop("s2-m78", _cfg(20, s=2), 5, 2, filt=_corners),
    *_coop("s2-m82", _cfg(21, s=2), 6, 2, filt=_corners),
    *_coop("s2-m112", _cfg(19, s=2), 7, 2, tw1=0),
    # ---- nd (by knob only), cell size 8
    _row("nd-m15", _cfg(8), "k_solve_nd<8,2>", "nd", filt=_corners),
    _row("nd-m23", _cfg(8), "k_solve_nd<8,3>", "nd"),
    _row("nd-m31", _cfg(8, l=2, nref=3), "k_solve_nd<8,4>", "nd", filt=_at_most_4_cells_wide),
]

# Instantiations of DESIGN.md's table that a test of another file launches (with the launch that does it)
COVERED_ELSEWHERE = {
    "k_solve_tw<2,1>": "test_gpu_parity.py::test_c1_all_patches (m_max 11)",
    "k_solve_nd<4,2>": "test_gpu_elasticity_and_quirks.py::test_nested_dissection_solver (n_sub 4, oversampling 1)",
    "k_solve_nd<4,3>": "test_gpu_elasticity_and_quirks.py::test_nested_dissection_solver (n_sub 4, oversampling 2)",
    "k_solve_nd<4,4>": "test_gpu_elasticity_and_quirks.py::test_nested_dissection_solver (n_sub 4, oversampling 3)",
    "k_solve_nd<8,5>": "test_gpu_elasticity_and_quirks.py::test_nested_dissection_solver (n_sub 8, oversampling 2)",
}

# The "reachable" part of DESIGN.md's table, literally: what tools/dump_solver_choice.cpp --instantiations
# reports as "auto" or "knob".  Not reachable (no row, DESIGN.md says why):
NEVER = {"k_solve_tw<2,2>", "k_solve<7,1,1>", "k_solve<7,2,1>", "k_solve_nd<4,5>"}
REACHABLE = (
    {"k_solve_tw<%d,1>" % t for t in (2, 3, 4, 5, 6, 8, 10, 12, 14)}
    | {"k_solve_tw<%d,2>" % t for t in (3, 4, 5, 6, 8, 10, 12, 14)}
    | {"k_solve_mf<%d,1>" % nt for nt in range(1, 8)}
    | {"k_solve_mf<%d,2>" % nt for nt in range(1, 6)}
    | {"k_solve<%d,1,%d>" % (r, tw) for r in range(1, 8) for tw in (0, 1) if (r, tw) != (7, 1)}
    | {"k_solve<%d,2,%d>" % (r, tw) for r in range(1, 8) for tw in (0, 1) if (r, tw) != (7, 1)}
    | {"k_solve_nd<%d,%d>" % (nv, t) for nv in (4, 8) for t in (2, 3, 4, 5) if (nv, t) != (4, 5)}
)

_LAUNCH = re.compile(r"\[slod\] (k_solve(?:_tw|_mf|_nd)?<[0-9,]+>)")


class _SharedOracle:
    """The oracle with its per-patch results kept: rows that share a configuration (one line width serves a
    tw, an mf and two coop rows) compute each reference once.  The arrays are read-only."""

    _store = {}

    def __init__(self, so, cfg):
        self._so = so
        self._key = tuple(getattr(cfg, f) for f, _ in cfg._fields_)

    def __getattr__(self, name):
        return getattr(self._so, name)

    def _memo(self, what, pid, fn):
        k = (self._key, what, pid)
        if k not in self._store:
            v = fn()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._store[k] = v
        return self._store[k]

    def patch_basis(self, cfg, fields, pid):
        return self._memo("basis", pid, lambda: self._so.patch_basis(cfg, fields, pid))

    def assemble_patch(self, cfg, fields, pid):
        return self._memo("stencil", pid, lambda: self._so.assemble_patch(cfg, fields, pid))

    def selection_conditioning(self, cfg, fields, pid):
        return self._memo("cond", pid, lambda: self._so.selection_conditioning(cfg, fields, pid))

    def patch_solution(self, cfg, fields, pid):
        return self._memo("X", pid, lambda: self._so.patch_debug(cfg, fields, pid)["X"])


def _plan_ids(g, filt):
    """One patch of every shape class (mx, my, side_domain) that passes the filter; all of them when they are
    at most 64."""
    shapes, ids = {}, []
    for pid in range(g.num_patches):
        i = g.patch_layout(pid)
        if filt(i):
            ids.append(pid)
            shapes.setdefault((i.mx, i.my, tuple(i.side_domain)), pid)
    if len(ids) > 64:
        ids = sorted(shapes.values())
    return np.array(ids, dtype=np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("env,kw,filt,expect", ROWS)
def test_instantiation_against_oracle(so, env, kw, filt, expect, monkeypatch, capfd):
    for k in ("SLOD_SOLVE", "SLOD_TWISTED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SLOD_DEBUG", "1")
    cfg, g = _mk(so, **kw)
    s = cfg.spacedim
    fields = make_fields(so, cfg, "D100")
    _upload(g, fields)
    ref = _SharedOracle(so, cfg)
    ids = _plan_ids(g, filt)
    assert len(ids) > 0
    m_max = max(s * (min(g.patch_layout(int(p)).mx, g.patch_layout(int(p)).my) * kw["n_sub"] - 1) for p in ids)
    capfd.readouterr()
    basis, premult, offs = g.compute_basis(ids)
    launched = set(_LAUNCH.findall(capfd.readouterr().err))
    assert launched == {expect}, "m_max %d: launched %s" % (m_max, sorted(launched))
    # (4) phi, psi of every patch of the plan
    worst_phi = worst_psi = 0.0
    for k, pid in enumerate(ids):
        ephi, epsi = _check_patch(ref, cfg, fields, int(pid), basis, premult, int(offs[k]), expect)
        worst_phi, worst_psi = max(worst_phi, ephi), max(worst_psi, epsi)
    # (5) the decisions of the selection stage (the plan path; its outputs are the host-buffer path's)
    dg = _decisions(g, ids, offs)
    checked = 0
    for k, pid in enumerate(ids):
        spread, stable = ref.selection_conditioning(cfg, fields, int(pid))
        if not stable:
            continue
        diag = ref.patch_basis(cfg, fields, int(pid))[2]
        for c in range(s):
            assert (dg[k * s + c].n_cut, dg[k * s + c].n_dropped) == (diag.n_cut[c], diag.n_dropped[c]), \
                "%s patch %d component %d: decisions gpu (%d,%d) oracle (%d,%d)" % (
                    expect, pid, c, dg[k * s + c].n_cut, dg[k * s + c].n_dropped, diag.n_cut[c], diag.n_dropped[c])
        checked += 1
    assert checked > 0
    # (6) X = A_II^-1 P_I^T itself, ahead of the selection stage (a one-patch plan: for a rim patch it may
    # launch a narrower instantiation than the plan's, so no log assertion here)
    worst_x = 0.0
    for pid in sorted({int(ids[0]), int(ids[-1])}):
        X = g.patch_solution(pid)
        xref = ref.patch_solution(cfg, fields, pid)
        assert np.isfinite(X).all()
        ex = np.abs(X - xref).max() / np.abs(xref).max()
        worst_x = max(worst_x, ex)
        assert ex <= TOL_X, "%s patch %d: |dX| / max|X| = %.3e" % (expect, pid, ex)
    print("INSTANTIATION %s m_max %d patches %d |dphi| %.3e |dpsi|/||A|| %.3e |dX|/max|X| %.3e"
          % (expect, m_max, len(ids), worst_phi, worst_psi, worst_x))


@pytest.mark.gpu
def test_coop_plan_beyond_the_lds_is_rejected_cleanly(monkeypatch):
    """SLOD_SOLVE=coop on a scalar plan of 111 dofs per line and 49 coarse dofs (n_sub 16, oversampling 3, a
    7 x 7-cell patch; plan creation only, nothing is launched): one chain alone needs
    (112^2 + 2 * 112 * 50 + 3 * 334) doubles = 193 KB of LDS.  The dispatcher drops the second chain, still has
    no fit and, the family being forced, offers no other kernel: slod_plan_create fails with
    SLOD_ERR_UNSUPPORTED.  Without the knob the same plan is created (tw)."""
    import slod_amd
    g = slod_amd.Slod(**_cfg(16, l=3, nref=3))
    full = [p for p in range(g.num_patches) if g.patch_layout(p).mx == 7 and g.patch_layout(p).my == 7]
    assert full
    ids = np.array(full[:1], dtype=np.uint32)
    monkeypatch.setenv("SLOD_SOLVE", "coop")
    for tw in ("0", "1"):
        monkeypatch.setenv("SLOD_TWISTED", tw)
        with pytest.raises(slod_amd.SlodError) as e:
            g.plan(ids)
        assert e.value.code == -2 and "LDS" in str(e.value)   # SLOD_ERR_UNSUPPORTED
    monkeypatch.delenv("SLOD_SOLVE")
    g.plan(ids).close()


def test_rows_cover_every_reachable_instantiation():
    """No GPU needed.  The rows above and the launches listed in COVERED_ELSEWHERE name exactly the reachable
    instantiations of DESIGN.md's table: a row deleted later, or an instantiation that becomes reachable
    without a row, fails here."""
    here = {p.values[3] for p in ROWS}
    assert here | set(COVERED_ELSEWHERE) == REACHABLE, (
        "missing: %s; not in the table: %s" % (sorted(REACHABLE - here - set(COVERED_ELSEWHERE)),
                                               sorted((here | set(COVERED_ELSEWHERE)) - REACHABLE)))
    assert not here & set(COVERED_ELSEWHERE)
    assert len(REACHABLE) == 62 and not REACHABLE & NEVER and len(REACHABLE | NEVER) == 66
    # the table itself
    import os
    from conftest import ROOT
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design.split("## Patch-solve instantiations", 1)[1]
    listed = {}
    for line in table.splitlines():
        m = re.match(r"\| `(k_solve[^`]*)` \| (auto|knob|never) \|", line)
        if m:
            listed[m.group(1)] = m.group(2)
    assert {n for n, r in listed.items() if r != "never"} == REACHABLE
    assert {n for n, r in listed.items() if r == "never"} == NEVER
