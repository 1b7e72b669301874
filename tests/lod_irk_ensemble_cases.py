"""Helpers of the tests of the implicit Runge-Kutta steppers on a coefficient ensemble
(slod_lod_irk_heat_steps_ensemble_direct, slod_lod_irk_wave_steps_ensemble_direct); a plain module like lod_irk_cases.py,
whose schemes, yardstick (heat_stage, wave_stage), growth cap and stage loads it shares.

Configurations, those of test_gpu_lod_ensemble_wave.py and built the same way (one handle with n_problems = 3, members
const / D100 / D1e4 of make_fields, one plan over all 3 * num_patches gids):
  base      nref 3, n_sub 2, l 1, s 1   64 rows
  s2        nref 3, n_sub 2, l 1, s 2   128 rows, elasticity
  rowmajor  5 cells, n_sub 3, l 1       25 rows, padding in n and b
K = 65 (base only) takes the scaled copies (1 + k/64) member[k mod 3] of A and of M alike: the pencil of a copy is that of
its member, its step matrix the member's times (1 + k/64), and 65 crosses a wave of 64 columns and the 64-column chunk of
the tiling.

Time steps: the rule of lod_irk_cases.py on the joint spectrum  lam_1 := max_k lam_1(k),  lam_n := max_k lam_n(k)  of the
members' dense pencils (scipy.linalg.eigh), so that the stiffest member sets the step as in the Newmark ensemble test:
  heat  0.1 / lam_1,  1 / sqrt(lam_1 lam_n),  10 / lam_1
  wave  0.5 / sqrt(lam_1),  0.05 / sqrt(lam_1),  2 / sqrt(lam_n)
Dampings: undamped and the three of lod_harmonic_cases.dampings at the joint lam_1.  The growth of every member's step
matrix <= GROWTH_CAP is a condition before the library is called (test_lod_irk_ensemble_reference.py checks it on the
CPU on surrogate pencils; the GPU test on the members' own).
"""
import numpy as np

import lod_irk_cases as ic
from lod_irk_cases import FORWARD, GAUSS, GROWTH_CAP, RADAU, SCHEMES   # noqa: F401

DISTS = ("const", "D100", "D1e4")
CONFIGS = {"base": dict(nref=3, n_sub=2, oversampling=1, spacedim=1),
           "s2": dict(nref=3, n_sub=2, oversampling=1, spacedim=2),
           "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1)}
ROWS = {"base": 64, "s2": 128, "rowmajor": 25}
NAMES = sorted(CONFIGS)
CASES = [(name, 3) for name in NAMES] + [("base", 65)]
CONTRASTS = (1.0, 100.0, 1e4)      # the three surrogate members of the CPU test


def joint_spectrum(lams):
    """(lam_1, lam_n) of the rule: the largest lowest and the largest highest eigenvalue over the members."""
    return np.array([max(float(l[0]) for l in lams), max(float(l[-1]) for l in lams)])


def heat_dts(lams):
    return ic.heat_dts(joint_spectrum(lams))


def wave_dts(lams):
    return ic.wave_dts(joint_spectrum(lams))


def wave_dampings(lams):
    """Undamped, then the three of lod_harmonic_cases.dampings at the joint lam_1."""
    return ic.wave_dampings(joint_spectrum(lams))


def scale(K, k, members=3):
    """The factor of member k of an ensemble of K: 1 for the members themselves, 1 + k/64 for the copies."""
    return 1.0 if k < members else 1.0 + k / 64.0


def surrogate_members():
    """[(A, M, lam)] of the Q1 surrogate at the three contrasts."""
    return [ic.q1_case(7, c)[:3] for c in CONTRASTS]


def problems(lams):
    """[(label, order, dt list, damp_mass, damp_stiff)]: heat, then the wave undamped and at each damping."""
    out = [("heat", 1, heat_dts(lams), 0.0, 0.0)]
    for label, dm, ds in wave_dampings(lams):
        out.append(("wave-" + label, 2, wave_dts(lams), dm, ds))
    return out


# ---- the three configurations with their members (needs a GPU)

_cache = {}


class _Ens:
    pass


def nan(*shape):
    from lod_cases import NAN, _torch
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def dev(a):
    from lod_cases import _torch
    torch, device = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def padded(a, pad):
    """[...][n + pad] device array with NaN in the padding columns."""
    t = nan(*a.shape[:-1], a.shape[-1] + pad)
    t[..., :a.shape[-1]] = dev(a)
    return t


def ens_case(so, name):
    """Handle, ensemble slab, and per member the single-problem sym(A), M and load vector (f = 1) on the device, the dense
    pencils with their spectra, the factor order; built once and left unchanged."""
    if name in _cache:
        return _cache[name]
    import scipy.linalg as sl
    import slod_amd
    from conftest import make_fields
    from lod_cases import _lod_matrix, _rows_to_dense, _torch
    from lod_ldl_cases import factor_order
    torch, device = _torch()
    kw = CONFIGS[name]
    c = _Ens()
    c.name, c.s, c.K = name, kw["spacedim"], len(DISTS)
    cfg = so.make_cfg(stabilize=1, **kw)
    g = c.g = slod_amd.Slod(nref=kw.get("nref", 0), n_sub=kw["n_sub"], oversampling=kw["oversampling"], spacedim=c.s,
                            n_cells=kw.get("n_cells", 0), n_problems=c.K)
    for k, dist in enumerate(DISTS):
        for f, a in enumerate(make_fields(so, cfg, dist)):
            g.set_coefficient(f, a, problem=k)
    NP = c.NP = g.num_patches
    plan = g.plan(np.arange(c.K * NP, dtype=np.uint32))
    c.stride = plan.stride
    c.mstride = NP * c.stride
    c.b = torch.zeros(c.K * c.mstride, dtype=torch.float64, device=device)
    c.q = torch.zeros_like(c.b)
    plan.execute(c.b.data_ptr(), c.q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    c.nrow, c.cap, c.field = NP * c.s, g.lod_row_capacity(), (g.NE + 1) ** 2 * c.s
    c.nval = NP * c.cap * c.s * c.s
    assert c.nrow == ROWS[name]
    c.slab = [(c.b[k * c.mstride:(k + 1) * c.mstride], c.q[k * c.mstride:(k + 1) * c.mstride]) for k in range(c.K)]
    c.values, c.cols = [], None
    for bk, qk in c.slab:
        v, cols = _lod_matrix(g, bk, qk, c.stride, c.s)
        c.values.append(v)
        assert c.cols is None or torch.equal(c.cols, cols)
        c.cols = cols
    hcols = c.cols.cpu().numpy().view(np.uint32)
    c.sym, c.mass = [], []
    for k in range(c.K):
        out = nan(c.nval)
        g.lod_matrix_symmetrize(c.values[k].data_ptr(), c.cols.data_ptr(), out.data_ptr())
        c.sym.append(out)
        out, mcols = nan(c.nval), torch.zeros_like(c.cols)
        g.lod_mass_matrix(np.arange(NP), c.slab[k][0].data_ptr(), c.stride, out.data_ptr(), mcols.data_ptr())
        c.mass.append(out)
    c.load = torch.zeros(c.field, dtype=torch.float64, device=device)
    g.fem_rhs(None, c.load.data_ptr())
    c.rhs = []
    for k in range(c.K):
        out = nan(c.nrow)
        g.lod_rhs(np.arange(NP), c.slab[k][0].data_ptr(), c.stride, c.load.data_ptr(), out.data_ptr())
        c.rhs.append(out)
    torch.cuda.synchronize()
    c.dA = [_rows_to_dense(g, v.contiguous().cpu().numpy(), hcols, c.s) for v in c.sym]
    c.dM = [_rows_to_dense(g, v.contiguous().cpu().numpy(), hcols, c.s) for v in c.mass]
    c.lam = [sl.eigh(c.dA[k], c.dM[k], eigvals_only=True) for k in range(c.K)]
    c.perm = factor_order(c)
    _cache[name] = c
    return c


def stack(c, mats, K, pad=0):
    """K matrices interleaved [nval][K + pad], NaN in the padding: the three members, then (1 + k/64) member[k mod 3]."""
    from lod_cases import _torch
    torch, _ = _torch()
    V = nan(c.nval, K + pad)
    V[:, :K] = torch.stack([mats[k % c.K] * scale(K, k, c.K) for k in range(K)], dim=1)
    return V


def member_dense(c, K, k):
    """(A, M) dense of member k of an ensemble of K, as stack() scales them."""
    f = scale(K, k, c.K)
    return c.dA[k % c.K] * f, c.dM[k % c.K] * f
