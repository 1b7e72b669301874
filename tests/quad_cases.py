"""The yardstick of the quad-parity tests, derived from references alone (a plain helper module like lod_cases.py,
not a conftest).

The truth is the oracle run in __float128 (slod_oracle.quad(), svd mode 0).  What fp64 can attain on a patch is
measured, not assumed: e64 is the largest distance from the truth over five fp64 restatements of the same
algorithm -- the oracle as it is, its svd mode 2 (the device's organisation of the selection: QR first), and the
oracle with a relative perturbation of 2**-50 (four ulp) on X = A^-1 P^T for three seeds, the least by which
any other fp64 solver differs.  The bar is

    tol_phi = max(1e-10, 10 * e64_phi),    tol_psi = max(1e-10, 10 * e64_psi) * ||A||_inf.

The floor is the project's bar (BASELINE north star).  The factor 10 is the one the parity tests already grant
over the oracle's own spread; here it multiplies an error measured against the truth instead of the movement
under a 1e-13 probe, which overstates that error a hundredfold.  It covers an operation order that none of the
five variants has.  Decisions (n_cut, n_dropped) are asserted on a patch when all five variants take the
truth's decisions.  Nothing in this module looks at a device result.

A case is (configuration, field), e.g. ("Q1", "D1e4"); everything is memoised per process by (case, patch), the
whole case at once on min(16, usable CPUs) threads (the C calls release the GIL)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import SEED, make_fields

FLOOR = 1e-10
FACTOR = 10.0
NOISE_EPS = 2.0 ** -50
NOISE_SEEDS = (1, 2, 3)

CONFIGS = {
    # stand-alone k_select<1>; register SVD path (4x7, 5x6) and LDS loops (35-49 columns); n_cut > 0 on most patches
    "Q1": dict(kw=dict(nref=3, n_sub=4, oversampling=3, spacedim=1), fields=("D100", "D1e4")),
    # the narrowest lines (13 dofs) with the same ill-conditioning
    "Q2": dict(kw=dict(nref=3, n_sub=2, oversampling=3, spacedim=1), fields=("D1e4",)),
    # k_solve_tw<5,1> with assembly and selection fused (C2's instantiation)
    "Q3": dict(kw=dict(nref=3, n_sub=8, oversampling=2, spacedim=1), fields=("D1e4",)),
    # elasticity, 50 columns; one patch per shape class, at most 16
    "Q4": dict(kw=dict(nref=3, n_sub=4, oversampling=2, spacedim=2), fields=("D1e4",), max_classes=16),
}
CASES = [(c, f) for c in ("Q1", "Q2", "Q3", "Q4") for f in CONFIGS[c]["fields"]]

# Patches on which an fp64 variant does not take the truth's decisions: dropped from the configuration by id, the
# reason being the truth's margins (printed by tests/test_oracle_quad.py).  At most 5 % per configuration.
DROPPED = {}

_setups = {}
_memo = {}     # (case, pid) -> entry, computed once and never modified
_extra = {}    # (case, what) -> per-case results of other runs (quad modes 1 and 2, X)


def nthreads():
    return min(16, len(os.sched_getaffinity(0)))


def _so():
    import slod_oracle
    slod_oracle.lib()
    return slod_oracle


def setup(case):
    """-> (cfg, fields) of the case."""
    if case not in _setups:
        so = _so()
        cfg = so.make_cfg(**CONFIGS[case[0]]["kw"])
        _setups[case] = (cfg, make_fields(so, cfg, case[1], SEED))
    return _setups[case]


def all_patches(case):
    """The patches the configuration runs, before DROPPED is taken out."""
    so = _so()
    cfg, _ = setup(case)
    n = so.num_patches(cfg)
    cap = CONFIGS[case[0]].get("max_classes")
    if cap is None:
        return list(range(n))
    first = {}
    for pid in range(n):
        p = so.patch_info(cfg, pid)
        first.setdefault((p.mx, p.my, tuple(p.side_domain)), pid)
    reps = sorted(first.values())
    if len(reps) > cap:   # evenly spread over the classes, the first (corner) and the last included
        reps = [reps[(i * (len(reps) - 1)) // (cap - 1)] for i in range(cap)]
    return reps


def patches(case):
    gone = set(DROPPED.get(case, ()))
    return [p for p in all_patches(case) if p not in gone]


def _decisions(diag, s):
    return tuple((diag.n_cut[c], diag.n_dropped[c]) for c in range(s))


def _map(fn, pids):
    with ThreadPoolExecutor(nthreads()) as pool:
        return list(pool.map(fn, pids))


def quad_run(case, mode=0):
    """{pid: (phi, psi, decisions, diag)} of the quad library in svd mode `mode`, every patch of the case."""
    key = (case, "quad%d" % mode)
    if key not in _extra:
        q = _so().quad()
        cfg, fields = setup(case)
        pids = all_patches(case)
        q.set_svd_mode(mode)
        try:
            res = _map(lambda pid: q.patch_basis(cfg, fields, pid), pids)
        finally:
            q.set_svd_mode(0)
        _extra[key] = {pid: (r[0], r[1], _decisions(r[2], cfg.spacedim), r[2]) for pid, r in zip(pids, res)}
    return _extra[key]


def fp64_variants(case):
    """[(name, {pid: (phi, psi, decisions)})] of the five fp64 variants."""
    key = (case, "fp64")
    if key not in _extra:
        so = _so()
        cfg, fields = setup(case)
        pids = all_patches(case)
        out = []
        settings = [("oracle", 0, 0.0, 0), ("svd_mode 2", 2, 0.0, 0)] + \
                   [("noise 2^-50 seed %d" % sd, 0, NOISE_EPS, sd) for sd in NOISE_SEEDS]
        try:
            for name, mode, eps, seed in settings:
                so.set_svd_mode(mode)
                so.set_solver_noise(eps, seed)
                res = _map(lambda pid: so.patch_basis(cfg, fields, pid), pids)
                out.append((name, {pid: (r[0], r[1], _decisions(r[2], cfg.spacedim)) for pid, r in zip(pids, res)}))
        finally:
            so.set_svd_mode(0)
            so.set_solver_noise(0.0, 0)
        _extra[key] = out
    return _extra[key]


def _ensure(case):
    if (case, "done") in _extra:
        return
    so = _so()
    cfg, fields = setup(case)
    tq = quad_run(case, 0)
    variants = fp64_variants(case)
    for pid in all_patches(case):
        phi_q, psi_q, dec_q, diag = tq[pid]
        a_inf = float(np.abs(so.assemble_patch(cfg, fields, pid)).sum(axis=(1, 3)).max())
        e_phi = max(float(np.abs(v[pid][0] - phi_q).max()) for _, v in variants)
        e_psi = max(float(np.abs(v[pid][1] - psi_q).max()) for _, v in variants) / a_inf
        s = cfg.spacedim
        for a in (phi_q, psi_q):
            a.setflags(write=False)
        _memo[(case, pid)] = dict(
            phi=phi_q, psi=psi_q, decisions=dec_q, a_inf=a_inf, e64_phi=e_phi, e64_psi=e_psi,
            margin_cut=min(diag.margin_cut[:s]), margin_half=min(diag.margin_half[:s]),
            asserted=all(v[pid][2] == dec_q for _, v in variants),
            disagree=[n for n, v in variants if v[pid][2] != dec_q])
    _extra[(case, "done")] = True


def truth(case, pid):
    """phi, psi (float64 roundings of the quad result, [s, n_f], read-only), decisions ((n_cut, n_dropped) per
    component), margin_cut, margin_half, a_inf."""
    _ensure(case)
    return _memo[(case, pid)]


def truth_x(case, pid):
    """X = A^-1 P^T of the quad library, [n_f, n_c]."""
    key = (case, "X", pid)
    if key not in _extra:
        cfg, fields = setup(case)
        x = _so().quad().patch_debug(cfg, fields, pid)["X"]
        x.setflags(write=False)
        _extra[key] = x
    return _extra[key]


def e64_phi(case, pid):
    return truth(case, pid)["e64_phi"]


def e64_psi(case, pid):
    """relative to ||A||_inf"""
    return truth(case, pid)["e64_psi"]


def tol_phi(case, pid):
    return max(FLOOR, FACTOR * e64_phi(case, pid))


def tol_psi(case, pid):
    t = truth(case, pid)
    return max(FLOOR, FACTOR * t["e64_psi"]) * t["a_inf"]


def decisions_asserted(case, pid):
    return truth(case, pid)["asserted"]


def old_bar(case, pid):
    """The widened bar of the parity tests that have no truth: max(1e-10, 10 * spread), the spread being how far the
    fp64 oracle moves under a 1e-13 probe on X (so.selection_conditioning).  -> (bar, spread, stable)"""
    key = (case, "old", pid)
    if key not in _extra:
        cfg, fields = setup(case)
        spread, stable = _so().selection_conditioning(cfg, fields, pid)
        _extra[key] = (max(FLOOR, 10.0 * spread), spread, stable)
    return _extra[key]


def worst_e64_patch(case):
    return max(patches(case), key=lambda pid: e64_phi(case, pid))
