#!/usr/bin/env python3
"""Time CG preconditioned by a banded factor next to the two solvers it joins, on BASELINE configuration C2 (2-D
Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 unknowns, half bandwidth 165, D1e4 coefficient), all in one run.

After a change of the coefficient in one coarse cell (its 8 x 8 fine elements times --factor, default 10; refreshed by
slod_update_coefficient, the dirty plan and slod_lod_matrix_update), for n_rhs = 1, 16, 64 on the refreshed system:
  (a) refactor     slod_lod_factor_create of the refreshed sym(A) plus slod_lod_factor_solve
  (b) jacobi       slod_lod_solve_multi
  (c) stale        slod_lod_solve_multi_precond with the factor of the matrix before the change
Then for K = 8 and 64 members (the D1e4 coefficient of K seeds, one load each):
  jacobi           slod_lod_solve_ensemble
  shared           slod_lod_solve_ensemble_precond with the factor of member 0 alone
  per_member       slod_lod_solve_ensemble_precond with slod_lod_factor_create_ensemble of all members (the factor timed
                   on its own)
rel_tol = 1e-12 everywhere.  Wall time of each synchronising call between two device synchronisations (they allocate
their workspace and read back inside; the factor of the run before is destroyed outside the timed region), after a
warm-up call: minimum, median and maximum of --reps runs.  One JSON line per measurement; nothing is asserted.

  python tools/lod_pcg_timing.py [--reps 7] [--factor 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-slod_amd"))

SEED = 20250614
C2 = dict(nref=5, n_sub=8, oversampling=2, spacedim=1, stabilize=1)
REL_TOL = 1e-12
MAX_IT = 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--factor", type=float, default=10.0)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_pcg_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    g = slod_amd.Slod(**C2)
    NP, cap, NE, n = g.num_patches, g.lod_row_capacity(), g.NE, C2["n_sub"]
    ids = np.arange(NP, dtype=np.uint32)
    plan = g.plan(ids)
    b = torch.zeros(NP * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)

    def spread(fn, before=None):
        """before: run ahead of every timed call, outside the timed region (it frees the factor of the call before)"""
        if before:
            before()
        fn()
        ms = []
        for _ in range(args.reps):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return {"min_ms": ms[0], "median_ms": ms[len(ms) // 2], "max_ms": ms[-1]}, out

    def matrix_of(field):
        """basis slabs and sym(A_LOD) of a coefficient field (numpy, per quadrature point)"""
        g.set_coefficient(0, field)
        plan.execute(b.data_ptr(), q.data_ptr())
        plan.status()
        raw, sym = torch.zeros(NP * cap, dtype=torch.float64, device=dev), torch.zeros(NP * cap, dtype=torch.float64, device=dev)
        g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
        g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), sym.data_ptr())
        torch.cuda.synchronize()
        return raw, sym

    def loads(kmax):
        g0 = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
        ey, ex, qq = np.meshgrid(np.arange(NE), np.arange(NE), np.arange(4), indexing="ij")
        xs = ((ex + np.where(qq & 1, 1.0 - g0, g0)) / NE).ravel()
        ys = ((ey + np.where(qq & 2, 1.0 - g0, g0)) / NE).ravel()
        nfine = (NE + 1) ** 2
        F = torch.zeros(kmax, nfine, dtype=torch.float64, device=dev)
        for k in range(kmax):
            fq = torch.from_numpy(np.sin((k + 1) * np.pi * xs) * np.sin(np.pi * ys)).to(dev)
            g.fem_rhs(fq.data_ptr(), F[k].data_ptr())
            torch.cuda.synchronize()
        B = torch.zeros(NP, kmax, dtype=torch.float64, device=dev)
        g.lod_rhs_multi(ids, b.data_ptr(), plan.stride, F.data_ptr(), nfine, kmax, B.data_ptr(), kmax)
        torch.cuda.synchronize()
        return B

    # ---- a change in one coarse cell, then three ways to solve the refreshed system
    field = fill_coefficient(SEED, "D1e4", NE)
    raw, sym_old = matrix_of(field)
    f_old = g.lod_factor(sym_old.data_ptr(), cols.data_ptr())
    cx = cy = (1 << C2["nref"]) // 2
    new = field.copy().reshape(NE, NE, 4)
    new[cy * n:(cy + 1) * n, cx * n:(cx + 1) * n, :] *= args.factor
    dirty = torch.zeros(NP, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.update_coefficient(0, new.ravel(), dirty.data_ptr())
    n_dirty = len(g.dirty_patches(dirty.data_ptr()))
    dplan = g.plan_dirty(dirty.data_ptr())
    dplan.execute(b.data_ptr(), q.data_ptr())
    dplan.status()
    torch.cuda.synchronize()
    g.lod_matrix_update(dirty.data_ptr(), b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr())
    sym = torch.zeros_like(sym_old)
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), sym.data_ptr())
    torch.cuda.synchronize()
    print(json.dumps({"change": "coarse cell (%d, %d) times %g" % (cx, cy, args.factor), "dirty_patches": n_dirty, "patches": NP,
                      "half_bandwidth": f_old.info.half_bandwidth, "reps": args.reps}), flush=True)
    Ball = loads(64)
    for nr in (1, 16, 64):
        B = Ball[:, :nr].contiguous()
        Ua, Ub, Uc = (torch.zeros_like(B) for _ in range(3))
        made = []

        def drop():
            while made:
                made.pop().close()

        def refactor():
            made.append(g.lod_factor(sym.data_ptr(), cols.data_ptr()))
            made[0].solve(B.data_ptr(), Ua.data_ptr(), n_rhs=nr)

        ta, _ = spread(refactor, before=drop)
        tb, (jit, _) = spread(lambda: g.lod_solve_multi(sym.data_ptr(), cols.data_ptr(), B.data_ptr(), nr, nr, Ub.data_ptr(), nr,
                                                       REL_TOL, MAX_IT))
        tc, (pit, pres) = spread(lambda: g.lod_solve_multi_precond(f_old, sym.data_ptr(), cols.data_ptr(), B.data_ptr(), nr, nr,
                                                                   Uc.data_ptr(), nr, REL_TOL, MAX_IT))
        scale = Ua.abs().max().item()
        print(json.dumps({"n_rhs": nr, "a_refactor_and_solve": ta, "b_jacobi_cg": tb, "c_stale_factor_pcg": tc,
                          "jacobi_iterations": [int(jit.min()), int(jit.max())], "pcg_iterations": [int(pit.min()), int(pit.max())],
                          "pcg_ms_per_iteration": tc["median_ms"] / max(int(pit.max()), 1),
                          "jacobi_ms_per_iteration": tb["median_ms"] / max(int(jit.max()), 1),
                          "pcg_vs_refactor_max_rel_difference": (Uc - Ua).abs().max().item() / scale,
                          "jacobi_vs_refactor_max_rel_difference": (Ub - Ua).abs().max().item() / scale}), flush=True)
        while made:
            made.pop().close()
    f_old.close()

    # ---- ensembles: K coefficients, one factor for all or one per member
    for K in (8, 64):
        V = torch.zeros(NP * cap, K, dtype=torch.float64, device=dev)
        for k in range(K):
            V[:, k] = matrix_of(fill_coefficient(SEED + 17 * k, "D1e4", NE))[1]
        B = loads(K)
        U = torch.zeros_like(B)
        first = V[:, 0].contiguous()
        torch.cuda.synchronize()
        shared = g.lod_factor(first.data_ptr(), cols.data_ptr())
        made = []

        def drop():
            while made:
                made.pop().close()

        def factor_all():
            made.append(g.lod_factor_ensemble(V.data_ptr(), cols.data_ptr(), K))

        tf, _ = spread(factor_all, before=drop)
        tj, (jit, _) = spread(lambda: g.lod_solve_ensemble(V.data_ptr(), cols.data_ptr(), B.data_ptr(), U.data_ptr(), K,
                                                          rel_tol=REL_TOL, max_iterations=MAX_IT))
        ts, (sit, _) = spread(lambda: g.lod_solve_ensemble_precond(shared, V.data_ptr(), cols.data_ptr(), B.data_ptr(), U.data_ptr(), K,
                                                                  rel_tol=REL_TOL, max_iterations=MAX_IT))
        tp, (mit, _) = spread(lambda: g.lod_solve_ensemble_precond(made[0], V.data_ptr(), cols.data_ptr(), B.data_ptr(), U.data_ptr(),
                                                                  K, rel_tol=REL_TOL, max_iterations=MAX_IT))
        print(json.dumps({"members": K, "jacobi_cg": tj, "shared_factor_pcg": ts, "per_member_factor_pcg": tp,
                          "factor_all_members": tf, "jacobi_iterations": [int(jit.min()), int(jit.max())],
                          "shared_iterations": [int(sit.min()), int(sit.max())],
                          "per_member_iterations": [int(mit.min()), int(mit.max())]}), flush=True)
        shared.close()
        while made:
            made.pop().close()


if __name__ == "__main__":
    main()
