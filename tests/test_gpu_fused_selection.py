"""GPU parity of the twisted solve with M = P^T A^-1 P / H^2 built inside its sweeps (default) and
with the selection stage computing M from X (SLOD_FUSE_M=0): phi to 1e-10, psi to 1e-10 * ||A||_inf
and the selection decisions equal to the oracle's, and which path each plan took."""
import numpy as np
import pytest

from conftest import make_fields

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _run(so, capfd, monkeypatch, fuse, ids=None, dist="D100", **kw):
    import slod_amd
    import torch
    monkeypatch.setenv("SLOD_DEBUG", "1")
    if fuse:
        monkeypatch.delenv("SLOD_FUSE_M", raising=False)
    else:
        monkeypatch.setenv("SLOD_FUSE_M", "0")
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
    b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    torch.cuda.synchronize()
    plan.status()
    err = capfd.readouterr().err
    dg = plan.diagnostics()
    hb, hq = b.cpu().numpy(), q.cpu().numpy()
    worst = 0.0
    for k, pid in enumerate(ids):
        p = so.patch_info(cfg, int(pid))
        phi, psi, diag = so.patch_basis(cfg, fields, int(pid))
        a_inf = np.abs(so.assemble_patch(cfg, fields, int(pid))).sum(axis=(1, 3)).max()
        off = k * plan.stride
        n = p.n_f
        ephi = np.abs(hb[off:off + n] - phi.ravel()).max()
        epsi = np.abs(hq[off:off + n] - psi.ravel()).max()
        assert ephi <= TOL, "patch %d fuse %d: |dphi| %.3e" % (pid, fuse, ephi)
        assert epsi <= TOL * a_inf, "patch %d fuse %d: |dpsi| %.3e" % (pid, fuse, epsi)
        if so.selection_conditioning(cfg, fields, int(pid))[1]: # decisions the oracle itself takes stably
            assert (dg[k].n_cut, dg[k].n_dropped) == (diag.n_cut[0], diag.n_dropped[0]), \
                "patch %d fuse %d: decisions gpu (%d,%d) oracle (%d,%d)" % (
                    pid, fuse, dg[k].n_cut, dg[k].n_dropped, diag.n_cut[0], diag.n_dropped[0])
        worst = max(worst, ephi)
    plan.close()
    return err, worst


def _path(err):
    """1: k_solve_tw built M in its sweeps, 0: it did not, None: another kernel ran"""
    lines = [ln for ln in err.splitlines() if "k_solve_tw<" in ln]
    if not lines:
        return None
    return int(lines[-1].rsplit("M in the sweeps", 1)[1])


def _c2_sample():
    # corners, edges (transposed and not), interior
    rim = [0, 1, 2, 31, 32, 33, 63, 96, 511, 512, 992, 1023, 1022, 990]
    return sorted(set(rim) | set(range(100, 1024, 37)))


SHAPES = [
    ("C1", dict(nref=3, n_sub=4, oversampling=1), None),
    ("C1-LOD", dict(nref=3, n_sub=4, oversampling=1, stabilize=0), None),
    ("n4-l1", dict(nref=4, n_sub=4, oversampling=1), None),
    ("n4-l2", dict(nref=4, n_sub=4, oversampling=2), None),
    ("n4-l3", dict(nref=4, n_sub=4, oversampling=3), None),
    ("C2-reuse", dict(nref=5, n_sub=8, oversampling=2, reuse_full=1), _c2_sample()),
]


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("name,kw,ids", SHAPES, ids=[s[0] for s in SHAPES])
def test_fused_m_shapes(so, capfd, monkeypatch, name, kw, ids, fuse):
    err, _ = _run(so, capfd, monkeypatch, fuse, ids=ids, **kw)
    path = _path(err)
    assert path is not None, "%s: the twisted kernel did not run:\n%s" % (name, err)
    if not fuse:
        assert path == 0
    elif name.startswith("C2") or name.startswith("C1"):
        assert path == 1, "%s: M was not built in the sweeps" % name


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("dist", ["D100", "D1e4"])
def test_fused_m_c2(so, capfd, monkeypatch, dist, fuse):
    err, worst = _run(so, capfd, monkeypatch, fuse, ids=_c2_sample(), dist=dist,
                      nref=5, n_sub=8, oversampling=2)
    assert _path(err) == fuse
    print("C2 %s fuse %d: worst |dphi| %.3e" % (dist, fuse, worst))


def test_fused_m_falls_back_on_wide_patches(so, capfd, monkeypatch):
    """C3 geometry (49 coarse columns): no M in the sweeps, the selection computes it from X."""
    err, _ = _run(so, capfd, monkeypatch, 1, ids=[48, 192], nref=4, n_sub=16, oversampling=3)
    assert _path(err) in (0, None)
