"""GPU checks of the SVD fallback of the selection stage on C2 (contrast 1e4), whose second-stage QR
picks its pivot column with a lane-parallel arg-max: the patches that take the fallback agree with
the oracle (phi to 1e-10, psi to 1e-10 * ||A||_inf, the project's tolerance; equal decisions where
the oracle itself decides stably), the fused launch and the stand-alone k_select give the same bits
(every wave searches on its own, so no result may depend on which wave is ahead), and so do two
executions of one plan."""
import numpy as np
import pytest

from conftest import make_fields

pytestmark = pytest.mark.gpu

TOL = 1e-10
KW = dict(nref=5, n_sub=8, oversampling=2)
MAX_ORACLE = 24 # fallback patches compared with the oracle (evenly spread over those found)


def _execute(g, ids, runs=1):
    import torch
    plan = g.plan(ids)
    dev = torch.device("cuda", 0)
    out = []
    for _ in range(runs):
        b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
        q = torch.zeros_like(b)
        plan.execute(b.data_ptr(), q.data_ptr())
        torch.cuda.synchronize()
        plan.status()
        out.append((b.cpu().numpy(), q.cpu().numpy()))
    dg = [(d.path, d.n_cut, d.n_dropped) for d in plan.diagnostics()]
    stride = plan.stride
    plan.close()
    return out, dg, stride


def _setup(so):
    import slod_amd
    cfg = so.make_cfg(**KW)
    g = slod_amd.Slod(device=0, **KW)
    fields = make_fields(so, cfg, "D1e4")
    for f, a in enumerate(fields):
        g.set_coefficient(f, a)
    return cfg, g, fields, np.arange(g.num_patches, dtype=np.uint32)


def test_fallback_patches_agree_with_oracle(so):
    cfg, g, fields, ids = _setup(so)
    (out,), dg, stride = _execute(g, ids)
    hb, hq = out
    # full patches (5 x 5 cells: 25 columns, so 24 pivot searches each) that took the SVD fallback
    slow = [k for k, pid in enumerate(ids)
            if dg[k][0] == 2 and (lambda i: i.mx == 5 and i.my == 5)(g.patch_layout(int(pid)))]
    assert len(slow) >= 8, "only %d full patches of C2/D1e4 took the SVD fallback" % len(slow)
    pick = [slow[i] for i in sorted(set(np.linspace(0, len(slow) - 1, MAX_ORACLE).astype(int)))]
    for k in pick:
        pid = int(ids[k])
        p = so.patch_info(cfg, pid)
        phi, psi, diag = so.patch_basis(cfg, fields, pid)
        a_inf = np.abs(so.assemble_patch(cfg, fields, pid)).sum(axis=(1, 3)).max()
        off, n = k * stride, p.n_f
        ephi = np.abs(hb[off:off + n] - phi.ravel()).max()
        epsi = np.abs(hq[off:off + n] - psi.ravel()).max()
        print("patch %d: |dphi| %.3e  |dpsi|/||A|| %.3e  decisions %s" % (pid, ephi, epsi / a_inf, dg[k][1:]))
        assert ephi <= TOL, "patch %d: |dphi| %.3e" % (pid, ephi)
        assert epsi <= TOL * a_inf, "patch %d: |dpsi| %.3e" % (pid, epsi)
        if so.selection_conditioning(cfg, fields, pid)[1]:
            assert dg[k][1:] == (diag.n_cut[0], diag.n_dropped[0]), \
                "patch %d: decisions gpu %s oracle (%d,%d)" % (pid, dg[k][1:], diag.n_cut[0], diag.n_dropped[0])


def test_fallback_is_bit_reproducible(so, monkeypatch):
    cfg, g, fields, ids = _setup(so)
    (r1, r2), dg1, _ = _execute(g, ids, runs=2)
    assert sum(1 for d in dg1 if d[0] == 2) >= 8
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]), "two executions of one plan differ"
    monkeypatch.setenv("SLOD_FUSE_SELECT", "0")
    (r0,), dg0, _ = _execute(g, ids)
    assert dg0 == dg1, "k_select and the fused selection stage decide differently"
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1]), "k_select and the fused stage differ"
