"""GPU tests of slod_compute_error_norms, the device counterpart of the error tables of the reference's
compare_lod_with_fem (LOD.cc:1240-1260), error_FEMh_exact (LOD.cc:1080-1088) and run() (LOD.cc:1425-1466):
L2, H1-seminorm and max-norm per component and the energy norm a(e,e)^{1/2}, all with the 2 x 2 Gauss rule
of the fine stiffness on every fine element."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_fields
from lod_cases import _exact_at_qp, _fem_reference, _gauss, _lod_matrix, _mk, _torch, _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")


def _np_norms(NE, s, e, fields, wq=None, wg=None):
    """numpy 2 x 2 Gauss integration of e = (nodal field) - w; returns squared sums (l2, h1, energy) and linf."""
    g = _gauss()
    h = 1.0 / NE
    jxw = 0.25 * h * h
    E = e.reshape(NE + 1, NE + 1, s)
    cn = [E[:-1, :-1], E[:-1, 1:], E[1:, :-1], E[1:, 1:]]           # corners (0,0) (1,0) (0,1) (1,1): [ey][ex][c]
    co = [f.reshape(NE, NE, 4) for f in fields]
    l2, h1, linf, en = np.zeros(s), np.zeros(s), np.zeros(s), 0.0
    for q in range(4):
        xi, eta = g[q & 1], g[q >> 1]
        N = [(1 - xi) * (1 - eta), xi * (1 - eta), (1 - xi) * eta, xi * eta]
        Gx = [-(1 - eta), 1 - eta, -eta, eta]
        Gy = [-(1 - xi), -xi, 1 - xi, xi]
        val = sum(N[a] * cn[a] for a in range(4))
        dx = sum(Gx[a] * cn[a] for a in range(4)) / h
        dy = sum(Gy[a] * cn[a] for a in range(4)) / h
        if wq is not None:
            val = val - np.moveaxis(wq.reshape(s, NE, NE, 4)[..., q], 0, -1)
            wgr = wg.reshape(s, 2, NE, NE, 4)
            dx = dx - np.moveaxis(wgr[:, 0, :, :, q], 0, -1)
            dy = dy - np.moveaxis(wgr[:, 1, :, :, q], 0, -1)
        l2 += (val ** 2).sum(axis=(0, 1)) * jxw
        h1 += (dx ** 2 + dy ** 2).sum(axis=(0, 1)) * jxw
        linf = np.maximum(linf, np.abs(val).max(axis=(0, 1)))
        if s == 1:
            en += (co[0][..., q] * (dx[..., 0] ** 2 + dy[..., 0] ** 2)).sum() * jxw
        else:
            e00, e11, e01 = dx[..., 0], dy[..., 1], 0.5 * (dy[..., 0] + dx[..., 1])
            en += (2 * co[1][..., q] * (e00 ** 2 + e11 ** 2 + 2 * e01 ** 2) + co[0][..., q] * (e00 + e11) ** 2).sum() * jxw
    return l2, h1, linf, en


def _random_nodal(NE, s, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.0, 1.0, (NE + 1, NE + 1, s))
    u[0], u[-1], u[:, 0], u[:, -1] = 0.0, 0.0, 0.0, 0.0
    return u.ravel()


CASES = [(dict(nref=3, n_sub=4, oversampling=1, spacedim=1), "D100"),
         (dict(nref=3, n_sub=4, oversampling=1, spacedim=1), "D1e4"),
         (dict(nref=2, n_sub=4, oversampling=1, spacedim=2), "D100")]


@pytest.mark.parametrize("kw,dist", CASES)
def test_error_norms_match_numpy_quadrature(so, kw, dist):
    """Random nodal fields with zero boundary values: L2, H1-seminorm and Linfty against a numpy 2 x 2 Gauss
    integration, energy^2 against e^T A e of the independently assembled fine stiffness (_fem_reference)."""
    torch, dev = _torch()
    cfg, g = _mk(so, stabilize=1, **kw)
    s = kw["spacedim"]
    fields = make_fields(so, cfg, dist)
    _upload(g, fields)
    hu, hv = _random_nodal(g.NE, s, 11), _random_nodal(g.NE, s, 12)
    u, v = torch.from_numpy(hu).to(dev), torch.from_numpy(hv).to(dev)
    r = g.error_norms(u.data_ptr(), v.data_ptr())
    l2, h1, linf, en = _np_norms(g.NE, s, hu - hv, fields)
    np.testing.assert_allclose(np.square(r["l2_components"]), l2, rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.square(r["h1_semi_components"]), h1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["linf_components"], linf, rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["energy"] ** 2, en, rtol=1e-12, atol=0)
    A, _, idx = _fem_reference(g.NE, s, fields)
    e = (hu - hv)[idx]
    np.testing.assert_allclose(r["energy"] ** 2, e @ (A @ e), rtol=1e-12, atol=0)
    # totals as ParsedConvergenceTable groups components of one name
    assert r["l2"] == pytest.approx(np.sqrt(l2.sum()), rel=1e-12)
    assert r["h1"] == pytest.approx(np.sqrt(l2.sum() + h1.sum()), rel=1e-12)
    assert r["linf"] == max(r["linf_components"])


@pytest.mark.parametrize("spacedim", [1, 2])
def test_error_norms_null_semantics_and_determinism(so, spacedim):
    torch, dev = _torch()
    cfg, g = _mk(so, nref=3, n_sub=4, oversampling=1, spacedim=spacedim, stabilize=1)
    _upload(g, make_fields(so, cfg, "D1e4"))
    hu, hv = _random_nodal(g.NE, spacedim, 21), _random_nodal(g.NE, spacedim, 22)
    u, v = torch.from_numpy(hu).to(dev), torch.from_numpy(hv).to(dev)
    d = (u - v).contiguous()
    torch.cuda.synchronize()
    zero = g.error_norms(u.data_ptr(), u.data_ptr())
    for k in ("l2", "h1_semi", "h1", "linf", "energy"):
        assert zero[k] == 0.0, (k, zero[k])
    both, diff = g.error_norms(u.data_ptr(), v.data_ptr()), g.error_norms(d.data_ptr())
    for k in ("l2", "h1_semi", "linf", "energy"):
        assert both[k] == pytest.approx(diff[k], rel=1e-14, abs=0), k
        assert both[k] > 0.0
    # v alone: e = -v
    neg = g.error_norms(None, v.data_ptr())
    only_v = g.error_norms(v.data_ptr())
    assert neg == only_v
    # bitwise repeatable, also on a non-default stream
    again = g.error_norms(u.data_ptr(), v.data_ptr())
    assert again == both
    side = torch.cuda.Stream()
    on_side = g.error_norms(u.data_ptr(), v.data_ptr(), stream=side.cuda_stream)
    on_torch = g.error_norms(u.data_ptr(), v.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert on_side == both and on_torch == both


def test_error_norms_need_the_coefficient(so):
    import slod_amd
    torch, dev = _torch()
    cfg, g = _mk(so, nref=2, n_sub=2, oversampling=1, stabilize=1)
    u = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    with pytest.raises(slod_amd.SlodError) as e:
        g.error_norms(u.data_ptr())
    assert e.value.code == -4
    _upload(g, make_fields(so, cfg, "D100"))
    assert g.error_norms(u.data_ptr())["energy"] == 0.0


def test_fem_error_against_exact_solution_converges(so):
    """error_FEMh_exact (LOD.cc:1080-1088): alpha = 1, u = sin(pi x) sin(pi y), f = 2 pi^2 u.  Fine FEM at
    NE = 16, 32, 64: the L2 error falls as h^2, the H1 seminorm error as h."""
    torch, dev = _torch()
    errs = []
    for nref in (2, 3, 4):
        cfg, g = _mk(so, nref=nref, n_sub=4, oversampling=1, stabilize=1)
        _upload(g, make_fields(so, cfg, "const"))
        w, wg, f = (torch.from_numpy(a).to(dev) for a in _exact_at_qp(g.NE))
        NEp = g.NE + 1
        rhs = torch.zeros(NEp * NEp, dtype=torch.float64, device=dev)
        uh = torch.zeros_like(rhs)
        g.fem_rhs(f.data_ptr(), rhs.data_ptr())
        it, res = g.fem_solve(rhs.data_ptr(), uh.data_ptr(), 1e-13, 50000)
        assert res <= 1e-12
        r = g.error_norms(uh.data_ptr(), None, w.data_ptr(), wg.data_ptr())
        # alpha = 1: the energy norm is the H1 seminorm
        assert r["energy"] == pytest.approx(r["h1_semi"], rel=1e-12)
        errs.append(r)
    for a, b in zip(errs[:-1], errs[1:]):
        assert 3.6 <= a["l2"] / b["l2"] <= 4.4, [e["l2"] for e in errs]
        assert 1.8 <= a["h1_semi"] / b["h1_semi"] <= 2.2, [e["h1_semi"] for e in errs]
    print("u_h - u: L2 %s, H1-semi %s" % (["%.3e" % e["l2"] for e in errs], ["%.3e" % e["h1_semi"] for e in errs]))


def _lod_vs_fem(so, g, fields, fem_tol=1e-12, lod_tol=1e-13):
    """The reference run() after the basis build (f = 1): returns (norms of u_h - u_LOD, norms of u_h)."""
    torch, dev = _torch()
    _upload(g, fields)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(ids)
    stride = plan.stride
    b = torch.zeros(len(ids) * stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    s = g.spacedim
    NEp = g.NE + 1
    f = torch.zeros(NEp * NEp * s, dtype=torch.float64, device=dev)
    g.fem_rhs(None, f.data_ptr())
    ufem = torch.zeros_like(f)
    g.fem_solve(f.data_ptr(), ufem.data_ptr(), fem_tol, 50000)
    values, cols = _lod_matrix(g, b, q, stride, s)
    rhs = torch.zeros(g.num_patches * s, dtype=torch.float64, device=dev)
    g.lod_rhs(ids, b.data_ptr(), stride, f.data_ptr(), rhs.data_ptr())
    uH = torch.zeros_like(rhs)
    g.lod_solve(values.data_ptr(), cols.data_ptr(), rhs.data_ptr(), uH.data_ptr(), lod_tol, 5000)
    ulod = torch.zeros_like(f)
    g.lod_reconstruct(b.data_ptr(), stride, uH.data_ptr(), ulod.data_ptr())
    return g.error_norms(ufem.data_ptr(), ulod.data_ptr()), g.error_norms(ufem.data_ptr())


def test_lod_error_decreases_with_oversampling(so):
    """compare_lod_with_fem in the norms of the method: relative L2 and energy errors of u_LOD against u_h
    (nref 3, n_sub 4, D100, SLOD) fall from l = 1 to l = 2."""
    rel = []
    for ell in (1, 2):
        cfg, g = _mk(so, nref=3, n_sub=4, oversampling=ell, stabilize=1)
        err, ref = _lod_vs_fem(so, g, make_fields(so, cfg, "D100"))
        rel.append((err["l2"] / ref["l2"], err["energy"] / ref["energy"]))
    assert rel[1][0] < rel[0][0] and rel[1][1] < rel[0][1], rel
    assert rel[1][0] < 2e-2, rel
    print("SLOD vs FEM(h), relative (L2, energy): l=1 %s, l=2 %s" % (rel[0], rel[1]))


def test_host_mirror_compare_matches_python_path(so):
    """bin/main_Diffusion 3 4 2 1 --compare runs the rest of the reference run() through the C++ mirror and
    prints the SLOD vs FEM(h) errors; they equal the Python path's on the same Alpha(1, 100, 3), srand(1)."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "--compare", "2", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    printed = {k: float(v) for k, v in re.findall(r"^\s*(L2|H1|Linfty|energy)\s+error = (\S+)", r.stdout, re.M)}
    assert set(printed) == {"L2", "H1", "Linfty", "energy"}, r.stdout
    assert "SLOD vs reference FEM(h)" in r.stdout
    plain = subprocess.run([BIN, "3", "4", "2", "1"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "SLOD vs" not in plain.stdout
    digest = [ln for ln in plain.stdout.splitlines() if ln.startswith("basis digest")]
    assert digest and digest[0] in r.stdout.splitlines()
    cfg, g = _mk(so, nref=3, n_sub=4, oversampling=2, stabilize=1)
    field = so.fill_coefficient_rand(1.0, 100.0, 3, g.NE, seed=1)
    err, _ = _lod_vs_fem(so, g, [field])
    assert printed["L2"] == pytest.approx(err["l2"], rel=1e-8)
    assert printed["H1"] == pytest.approx(err["h1"], rel=1e-8)
    assert printed["energy"] == pytest.approx(err["energy"], rel=1e-8)
