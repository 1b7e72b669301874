#!/usr/bin/env python3
"""Time an outer iteration of slod_lod_eigs on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8, oversampling
2: 1024 patches = 1024 rows, 49 slots per block row, D1e4 coefficient), for n_eig = 8 (12 block columns) and for the
widest block (n_eig = 48, 64 columns).

An outer iteration is  Y = M X,  A Z = Y (multi-column CG),  W = A Z,  V = M Z,  then the three kernels of
slod_lod_eig.hip (Gram, Ritz, rotate) and a read-back of 2 n_block + 1 words.  The ABI exposes the first four steps as
calls of their own, so the split is measured as
  outer     HIP-event time of slod_lod_eigs with max_outer = --outer, divided by the outer iterations it ran
  solve     slod_lod_solve_multi on Y = M X of the start block, same inner tolerance (the first inner solve)
  products  three slod_lod_apply_multi calls
  ritz      outer - solve - products: Gram, Ritz, rotate, residual and the read-back
(median of --reps after a warm-up).  The inner solves of later outer iterations start from other right-hand sides, so
`ritz` is an estimate, not a kernel time: for per-kernel times run this script under a kernel trace.  No time is
asserted anywhere.  The bytes each new kernel must move at least once (nrow rows, m columns, 8-byte words):
  gram     reads Z, W, V: 3 nrow m;  writes 2 m^2 per slab of 32 rows, which the ordered sum reads twice
  ritz     reads 2 m^2, writes m^2 + m
  rotate   reads Z, W, V and m^2 per block;  writes X: nrow m, and 2 m per slab of 16 rows
One JSON line per measurement.

  python tools/lod_eig_timing.py [--reps 5] [--outer 4]
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
INNER_TOL = 1e-12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outer", type=int, default=4)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_eig_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    g = slod_amd.Slod(**C2)
    t = torch.from_numpy(fill_coefficient(SEED, "D1e4", g.NE)).to(dev)
    g.set_coefficient_device(0, t.data_ptr(), t.numel())
    ids = np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(ids)
    b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    NP, cap = g.num_patches, g.lod_row_capacity()
    nrow = NP
    raw = torch.zeros(NP * cap, dtype=torch.float64, device=dev)
    values, mvalues = torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mvalues.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), values.data_ptr())
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    def median(fn):
        fn()
        return sorted(timed(fn)[:2] for _ in range(args.reps))[args.reps // 2]

    for n_eig, m in ((8, 12), (48, 64)):
        X = torch.zeros(nrow, m, dtype=torch.float64, device=dev)
        Y, Z, W, V = (torch.zeros_like(X) for _ in range(4))

        def eigs(max_outer=args.outer):
            return g.lod_eigs(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                              max_outer=max_outer, inner_rel_tol=INNER_TOL, inner_max_iterations=20000)

        t_outer = median(eigs)
        lam, res, its = eigs()
        eigs(1)                                        # X = the block after one outer iteration
        g.lod_apply(mvalues.data_ptr(), cols.data_ptr(), X.data_ptr(), Y.data_ptr(), n_rhs=m)

        def solve():
            return g.lod_solve_multi(values.data_ptr(), cols.data_ptr(), Y.data_ptr(), m, m, Z.data_ptr(), m, INNER_TOL, 20000)

        def products():
            g.lod_apply(mvalues.data_ptr(), cols.data_ptr(), X.data_ptr(), Y.data_ptr(), n_rhs=m)
            g.lod_apply(values.data_ptr(), cols.data_ptr(), Z.data_ptr(), W.data_ptr(), n_rhs=m)
            g.lod_apply(mvalues.data_ptr(), cols.data_ptr(), Z.data_ptr(), V.data_ptr(), n_rhs=m)

        t_solve, t_prod = median(solve), median(products)
        sit, _ = solve()
        per_outer = t_outer[0] / len(its)
        n_gslab, n_rslab = (nrow + 31) // 32, (nrow + 15) // 16
        n_rblock = min(n_rslab, 1024)
        print(json.dumps({
            "n_eig": n_eig, "n_block": m, "rows": nrow, "outer_run": len(its), "inner_iterations": its.tolist(),
            "eigs_event_ms": t_outer[0], "eigs_wall_ms": t_outer[1], "event_ms_per_outer": per_outer,
            "solve_event_ms": t_solve[0], "solve_iterations_max": int(sit.max()), "products_event_ms": t_prod[0],
            "ritz_estimate_ms": per_outer - t_solve[0] - t_prod[0],
            "ritz_estimate_share": (per_outer - t_solve[0] - t_prod[0]) / per_outer,
            "gram_bytes": 8 * (3 * nrow * m + 2 * m * m * n_gslab * 3), "ritz_bytes": 8 * (3 * m * m + m),
            "rotate_bytes": 8 * (3 * nrow * m + m * m * n_rblock + nrow * m + 2 * m * n_rslab),
            "lambda_1": float(lam[0]), "max_residual_of_n_eig": float(res[:n_eig].max())}), flush=True)


if __name__ == "__main__":
    main()
