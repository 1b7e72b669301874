#!/usr/bin/env python3
"""Time an outer iteration of slod_lod_eigs_direct next to one of slod_lod_eigs, and the ensemble call next to K single
calls, on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 patches = 1024 rows, 49 slots
per block row, D1e4 coefficient), for n_eig = 8 (12 block columns) and for the widest block (n_eig = 48, 64 columns).

An outer iteration of the direct call is  Y = M X,  S Z = Y (the two sweeps of the banded Cholesky factor of S = sym(A)),
W = A Z,  V = M Z,  then Gram, Ritz, rotate, residual and a read-back of 2 n_block + 2 words.  The ABI exposes the first
four steps as calls of their own, so the split is measured as
  outer     HIP-event time of the call with max_outer = --outer and a tol nothing reaches, divided by --outer
  solve     slod_lod_factor_solve on n_block columns
  products  three slod_lod_apply_multi calls (the call itself runs the same fma chain in k_eig_apply)
  ritz      outer - solve - products: Gram, Ritz, rotate, residual and the read-back
(median of --reps after a warm-up).  `ritz` is an estimate, not a kernel time: for per-kernel times run this script under
a kernel trace.  slod_lod_eigs runs on the same matrices with the same block, inner tolerance 1e-12, for the same number
of outer iterations.
The ensemble: K = 1, 8, 64 members, the matrices of member k are (1 + k/64) times those of the C2 pencil (the spectrum
of every member is that of the pencil, so every member does the same work), one ensemble factor and one call against K
single factors and K calls in sequence, --outer iterations each.
No time is asserted anywhere.  One JSON line per measurement.

  python tools/lod_eig_direct_timing.py [--reps 5] [--outer 4]
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
NEVER = 1e-300        # a tol no residual reaches: every call runs max_outer iterations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outer", type=int, default=4)
    ap.add_argument("--members", type=int, nargs="*", default=[1, 8, 64])
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_eig_direct_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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

    t_factor = median(lambda: g.lod_factor(values.data_ptr(), cols.data_ptr()).close())
    f = g.lod_factor(values.data_ptr(), cols.data_ptr())
    for n_eig, m in ((8, 12), (48, 64)):
        X = torch.zeros(nrow, m, dtype=torch.float64, device=dev)
        Y, Z, W, V = (torch.zeros_like(X) for _ in range(4))

        def direct(max_outer=args.outer, tol=NEVER):
            return g.lod_eigs_direct(f, values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                                     max_outer=max_outer, tol=tol)

        def cg():
            return g.lod_eigs(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                              max_outer=args.outer, tol=NEVER, inner_rel_tol=INNER_TOL, inner_max_iterations=20000)

        t_cg = median(cg)
        its = cg()[2]
        t_direct = median(direct)
        lam, res, outer = direct(200, 1e-10)            # to convergence, for the record
        direct(1)                                       # X = the block after one outer iteration
        g.lod_apply(mvalues.data_ptr(), cols.data_ptr(), X.data_ptr(), Y.data_ptr(), n_rhs=m)

        def solve():
            f.solve(Y.data_ptr(), Z.data_ptr(), n_rhs=m)

        def products():
            g.lod_apply(mvalues.data_ptr(), cols.data_ptr(), X.data_ptr(), Y.data_ptr(), n_rhs=m)
            g.lod_apply(values.data_ptr(), cols.data_ptr(), Z.data_ptr(), W.data_ptr(), n_rhs=m)
            g.lod_apply(mvalues.data_ptr(), cols.data_ptr(), Z.data_ptr(), V.data_ptr(), n_rhs=m)

        t_solve, t_prod = median(solve), median(products)
        per_outer = t_direct[0] / args.outer
        print(json.dumps({
            "n_eig": n_eig, "n_block": m, "rows": nrow, "outer": args.outer,
            "direct_event_ms_per_outer": per_outer, "direct_wall_ms": t_direct[1],
            "cg_event_ms_per_outer": t_cg[0] / len(its), "cg_inner_iterations": its.tolist(),
            "factor_create_event_ms": t_factor[0], "factor_bytes": int(f.info.bytes), "half_bandwidth": int(f.info.half_bandwidth),
            "solve_event_ms": t_solve[0], "products_event_ms": t_prod[0],
            "ritz_estimate_ms": per_outer - t_solve[0] - t_prod[0],
            "ritz_estimate_share": (per_outer - t_solve[0] - t_prod[0]) / per_outer,
            "outer_to_1e-10": int(outer), "lambda_1": float(lam[0]), "max_residual_of_n_eig": float(res[:n_eig].max())}), flush=True)

        for K in args.members:
            scale = torch.tensor([1.0 + k / 64.0 for k in range(K)], dtype=torch.float64, device=dev)
            A = (values[:, None] * scale[None, :]).contiguous()
            M = (mvalues[:, None] * scale[None, :]).contiguous()
            fe = g.lod_factor_ensemble(A.data_ptr(), cols.data_ptr(), K)
            XE = torch.zeros(nrow, K * m, dtype=torch.float64, device=dev)
            singles = []
            for k in range(K):
                Ak, Mk = A[:, k].contiguous(), M[:, k].contiguous()
                singles.append((Ak, Mk, g.lod_factor(Ak.data_ptr(), cols.data_ptr())))

            def ensemble():
                return g.lod_eigs_ensemble_direct(fe, A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, n_eig, XE.data_ptr(), n_block=m,
                                                  max_outer=args.outer, tol=NEVER)

            def sequence():
                for Ak, Mk, fk in singles:
                    g.lod_eigs_direct(fk, Ak.data_ptr(), Mk.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                                      max_outer=args.outer, tol=NEVER)

            t_ens, t_seq = median(ensemble), median(sequence)
            print(json.dumps({
                "n_eig": n_eig, "n_block": m, "rows": nrow, "members": K, "outer": args.outer,
                "ensemble_event_ms_per_outer": t_ens[0] / args.outer, "ensemble_wall_ms": t_ens[1],
                "sequence_event_ms_per_outer": t_seq[0] / args.outer, "sequence_wall_ms": t_seq[1],
                "sequence_over_ensemble": t_seq[0] / t_ens[0]}), flush=True)
            for _, _, fk in singles:
                fk.close()
            fe.close()
    f.close()


if __name__ == "__main__":
    main()
