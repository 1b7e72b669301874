"""GPU parity of k_solve_tw's backward sweep with K of X_l = Z_l - V_l Y split between the two waves
of a chain (default) and with the column-tile split (SLOD_BWD_KSPLIT=0): X to 1e-11 * max|X|, phi to
1e-10, psi to 1e-10 * ||A||_inf, selection decisions equal to the oracle's where the oracle takes them
stably, which path each plan took, repeatability, and on/off agreement to 1e-12 in phi (the two differ
only by summation order; 1e-12 is 4x the worst GPU-vs-oracle |dphi| 2.5e-13 recorded in DESIGN.md
section 5)."""
import numpy as np
import pytest

from conftest import make_fields

pytestmark = pytest.mark.gpu

TOL = 1e-10
C2 = dict(nref=5, n_sub=8, oversampling=2)

_oracle_cache = {}


def _switch(monkeypatch, ksplit):
    monkeypatch.setenv("SLOD_DEBUG", "1")
    if ksplit:
        monkeypatch.delenv("SLOD_BWD_KSPLIT", raising=False)
    else:
        monkeypatch.setenv("SLOD_BWD_KSPLIT", "0")


def _path(err):
    """1: the K-split loop ran, 0: the column-split / generic loop, None: another kernel ran"""
    lines = [ln for ln in err.splitlines() if "k_solve_tw<" in ln]
    if not lines:
        return None
    return int(lines[-1].rsplit("backward K split", 1)[1].split(",")[0])


def _oracle(so, cfg, fields, key, pid):
    k = (key, int(pid))
    if k not in _oracle_cache:
        p = so.patch_info(cfg, int(pid))
        phi, psi, diag = so.patch_basis(cfg, fields, int(pid))
        a_inf = np.abs(so.assemble_patch(cfg, fields, int(pid))).sum(axis=(1, 3)).max()
        stable = bool(so.selection_conditioning(cfg, fields, int(pid))[1])
        _oracle_cache[k] = (p.n_f, phi.ravel().copy(), psi.ravel().copy(), a_inf, stable,
                            (diag.n_cut[0], diag.n_dropped[0]))
    return _oracle_cache[k]


def _execute(so, capfd, monkeypatch, ksplit, ids=None, dist="D100", repeat=1, **kw):
    """Runs one plan (repeat executes); returns stderr, stride, the outputs of each execute, diagnostics."""
    import slod_amd
    import torch
    _switch(monkeypatch, ksplit)
    cfg = so.make_cfg(**kw)
    g = slod_amd.Slod(device=0, **kw)
    fields = make_fields(so, cfg, dist)
    for f, a in enumerate(fields):
        g.set_coefficient(f, a)
    if ids is None:
        ids = np.arange(g.num_patches)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    capfd.readouterr()
    plan = g.plan(ids)
    dev = torch.device("cuda", 0)
    outs = []
    for _ in range(repeat):
        b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
        q = torch.zeros_like(b)
        plan.execute(b.data_ptr(), q.data_ptr())
        torch.cuda.synchronize()
        plan.status()
        outs.append((b.cpu().numpy(), q.cpu().numpy()))
    err = capfd.readouterr().err
    dg = plan.diagnostics()
    decisions = [(dg[k].n_cut, dg[k].n_dropped) for k in range(len(ids))]
    stride = plan.stride
    plan.close()
    return cfg, fields, ids, err, stride, outs, decisions


def _check_against_oracle(so, cfg, fields, key, ids, stride, out, decisions, label):
    hb, hq = out
    worst = 0.0
    for k, pid in enumerate(ids):
        n, phi, psi, a_inf, stable, dec = _oracle(so, cfg, fields, key, pid)
        off = k * stride
        ephi = np.abs(hb[off:off + n] - phi).max()
        epsi = np.abs(hq[off:off + n] - psi).max()
        assert ephi <= TOL, "%s patch %d: |dphi| %.3e" % (label, pid, ephi)
        assert epsi <= TOL * a_inf, "%s patch %d: |dpsi| %.3e" % (label, pid, epsi)
        if stable:  # decisions the oracle itself takes stably
            assert decisions[k] == dec, "%s patch %d: decisions gpu %s oracle %s" % (label, pid, decisions[k], dec)
        worst = max(worst, ephi)
    return worst


def _c2_shape_patches(so, cfg, n_patches):
    """The first and the last patch of every C2 shape class: 3, 4 or 5 coarse cells per side (distance
    0, 1, >= 2 from the domain boundary), both orientations -- so transposed patches and chain pairs
    of unequal length (even number of lines) are covered."""
    first, last = {}, {}
    for pid in range(n_patches):
        p = so.patch_info(cfg, pid)
        first.setdefault((p.mx, p.my), pid)
        last[(p.mx, p.my)] = pid
    assert set(first) == {(a, b) for a in (3, 4, 5) for b in (3, 4, 5)}
    return sorted(set(first.values()) | set(last.values()))


@pytest.mark.parametrize("ksplit", [1, 0])
def test_patch_solution_c2_shape_classes(so, capfd, monkeypatch, ksplit):
    import slod_amd
    _switch(monkeypatch, ksplit)
    cfg = so.make_cfg(**C2)
    g = slod_amd.Slod(device=0, **C2)
    fields = make_fields(so, cfg, "D100")
    for f, a in enumerate(fields):
        g.set_coefficient(f, a)
    for pid in _c2_shape_patches(so, cfg, g.num_patches):
        capfd.readouterr()
        X = g.patch_solution(pid)
        assert _path(capfd.readouterr().err) == ksplit
        ref = so.patch_debug(cfg, fields, pid)["X"]
        e = np.abs(X - ref).max() / np.abs(ref).max()
        info = so.patch_info(cfg, pid)
        print("ksplit %d patch %d (%d x %d cells): |dX| / max|X| = %.3e" % (ksplit, pid, info.mx, info.my, e))
        assert e <= 1e-11, "ksplit %d patch %d: |dX| %.3e" % (ksplit, pid, e)


# Edges of the scheme: nc <= 16 (one column tile: the second wave only hands over its partial); m not a
# multiple of 16 or of the tile; m just under 48 (three full row tiles); LOD branch
EDGE_SHAPES = [
    ("nc9-m11", dict(nref=3, n_sub=4, oversampling=1), None),
    ("nc9-m11-LOD", dict(nref=3, n_sub=4, oversampling=1, stabilize=0), None),
    ("nc25-m19", dict(nref=4, n_sub=4, oversampling=2), None),
    ("nc9-m47", dict(nref=3, n_sub=16, oversampling=1), [0, 3, 9, 27, 36, 63]),
    ("nc9-m17", dict(nref=3, n_sub=6, oversampling=1), [0, 5, 9, 18, 62]),
    ("nc25-m34", dict(nref=3, n_sub=7, oversampling=2), [0, 1, 10, 27, 63]),
]


@pytest.mark.parametrize("ksplit", [1, 0])
@pytest.mark.parametrize("name,kw,ids", EDGE_SHAPES, ids=[s[0] for s in EDGE_SHAPES])
def test_edge_shapes(so, capfd, monkeypatch, name, kw, ids, ksplit):
    cfg, fields, ids, err, stride, outs, dec = _execute(so, capfd, monkeypatch, ksplit, ids=ids, **kw)
    assert _path(err) == ksplit, "%s: path\n%s" % (name, err)
    worst = _check_against_oracle(so, cfg, fields, (name, "D100"), ids, stride, outs[0], dec,
                                  "%s ksplit %d" % (name, ksplit))
    print("%s ksplit %d: worst |dphi| %.3e" % (name, ksplit, worst))


def test_wide_plans_take_the_old_path(so, capfd, monkeypatch):
    """C3 geometry (49 coarse columns, m = 111): no K split, whatever the switch says."""
    cfg, fields, ids, err, stride, outs, dec = _execute(so, capfd, monkeypatch, 1, ids=[48, 192],
                                                        nref=4, n_sub=16, oversampling=3)
    assert _path(err) in (0, None), err
    _check_against_oracle(so, cfg, fields, ("C3", "D100"), ids, stride, outs[0], dec, "C3")


@pytest.mark.parametrize("dist", ["D100", "D1e4"])
def test_c2_all_patches_on_and_off(so, capfd, monkeypatch, dist):
    """All 1024 patches of C2 with the switch on and off against the oracle; two executes of one plan
    bit-identical; on and off agree to 1e-12 in phi."""
    res = {}
    for ksplit in (1, 0):
        cfg, fields, ids, err, stride, outs, dec = _execute(so, capfd, monkeypatch, ksplit, dist=dist, repeat=2, **C2)
        assert _path(err) == ksplit
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), \
            "ksplit %d: two executes of the same plan differ" % ksplit
        worst = _check_against_oracle(so, cfg, fields, ("C2", dist), ids, stride, outs[0], dec,
                                      "C2/%s ksplit %d" % (dist, ksplit))
        print("C2 %s ksplit %d: worst |dphi| %.3e" % (dist, ksplit, worst))
        res[ksplit] = outs[0]
    d = np.abs(res[1][0] - res[0][0]).max()
    print("C2 %s: on vs off max |dphi| %.3e" % (dist, d))
    assert d <= 1e-12, "C2 %s: on and off differ by %.3e in phi" % (dist, d)
