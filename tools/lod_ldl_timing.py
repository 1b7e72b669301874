#!/usr/bin/env python3
"""Time the banded LDL^T factor next to the banded Cholesky factor, and an outer iteration of
slod_lod_eigs_shift_direct, on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 patches =
1024 rows, half bandwidth 165, D1e4 coefficient).

  factor    slod_lod_factor_create on sym(A) (the entry point of the parent, in this process), slod_lod_factor_create_ldl
            on the same definite matrix and on S = sym(A) - sigma M with sigma in the gap above the 8th eigenvalue (found
            by slod_lod_eigs_direct); the LDL^T call also runs k_ldl_norms twice and reads two more words back
  solve     slod_lod_factor_solve on the Cholesky factor of sym(A) and on the LDL^T factor of S, 12 and 64 columns
  outer     slod_lod_eigs_shift_direct on the LDL^T factor of S with max_outer = --outer and a tol nothing reaches,
            divided by --outer, next to slod_lod_eigs_direct on the Cholesky factor of sym(A); then the shift call to
            convergence, for the record, with the inertia and the growth of the factor
HIP-event times, the median of --reps after a warm-up.  No time is asserted anywhere.  One JSON line per measurement,
printed and, with --out, appended to that file.

  python tools/lod_ldl_timing.py [--reps 5] [--outer 4] [--out profiles/r21_lod_ldl_timing.jsonl]
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
NEVER = 1e-300        # a tol no residual reaches: every call runs max_outer iterations
BELOW = 8             # sigma sits in the gap above this many eigenvalues


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outer", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_ldl_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    values, mvalues, shifted = torch.zeros_like(raw), torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mvalues.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), values.data_ptr())
    torch.cuda.synchronize()

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

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

    # sigma: the midpoint of the gap above the BELOW-th eigenvalue
    fc = g.lod_factor(values.data_ptr(), cols.data_ptr())
    m0 = BELOW + 8
    X = torch.zeros(nrow, 64, dtype=torch.float64, device=dev)
    low = g.lod_eigs_direct(fc, values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), BELOW + 1, X.data_ptr(), n_block=m0, ld_x=64)[0]
    sigma = 0.5 * float(low[BELOW - 1] + low[BELOW])
    g.lod_matrix_combine(1.0, values.data_ptr(), -sigma, mvalues.data_ptr(), shifted.data_ptr())
    torch.cuda.synchronize()

    t_chol = median(lambda: g.lod_factor(values.data_ptr(), cols.data_ptr()).close())
    t_ldl_def = median(lambda: g.lod_factor_ldl(values.data_ptr(), cols.data_ptr()).close())
    t_ldl = median(lambda: g.lod_factor_ldl(shifted.data_ptr(), cols.data_ptr()).close())
    fl = g.lod_factor_ldl(shifted.data_ptr(), cols.data_ptr())
    ine = fl.inertia()
    emit({"rows": nrow, "half_bandwidth": int(fl.info.half_bandwidth), "sigma": sigma, "n_negative": int(ine.n_negative),
          "growth": ine.growth, "norm_matrix": ine.norm_matrix, "norm_factor": ine.norm_factor,
          "min_abs_pivot": ine.min_abs_pivot, "max_abs_pivot": ine.max_abs_pivot,
          "cholesky_create_event_ms": t_chol[0], "cholesky_create_wall_ms": t_chol[1],
          "ldl_create_definite_event_ms": t_ldl_def[0], "ldl_create_definite_wall_ms": t_ldl_def[1],
          "ldl_create_shifted_event_ms": t_ldl[0], "ldl_create_shifted_wall_ms": t_ldl[1],
          "cholesky_bytes": int(fc.info.bytes), "ldl_bytes": int(fl.info.bytes)})

    for n in (12, 64):
        B = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 1.0, (nrow, n))).to(dev)
        Uc, Ul = torch.zeros_like(B), torch.zeros_like(B)
        t_sc = median(lambda: fc.solve(B.data_ptr(), Uc.data_ptr(), n_rhs=n))
        t_sl = median(lambda: fl.solve(B.data_ptr(), Ul.data_ptr(), n_rhs=n))
        emit({"rows": nrow, "n_rhs": n, "cholesky_solve_event_ms": t_sc[0], "ldl_solve_event_ms": t_sl[0],
              "ldl_over_cholesky": t_sl[0] / t_sc[0]})

    for n_eig, m in ((8, 12), (48, 64)):
        def shift(max_outer=args.outer, tol=NEVER):
            return g.lod_eigs_shift_direct(fl, sigma, values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(),
                                           n_block=m, ld_x=64, max_outer=max_outer, tol=tol)

        def lowest():
            return g.lod_eigs_direct(fc, values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(), n_block=m, ld_x=64,
                                     max_outer=args.outer, tol=NEVER)

        t_shift, t_low = median(shift), median(lowest)
        lam, res, outer = shift(400, 1e-10)
        emit({"n_eig": n_eig, "n_block": m, "rows": nrow, "outer": args.outer, "sigma": sigma,
              "shift_event_ms_per_outer": t_shift[0] / args.outer, "shift_wall_ms": t_shift[1],
              "direct_event_ms_per_outer": t_low[0] / args.outer,
              "outer_to_1e-10": int(outer), "below_sigma_of_n_eig": int((lam[:n_eig] < sigma).sum()),
              "nearest": [float(v) for v in lam[:min(n_eig, 4)]], "max_residual_of_n_eig": float(res[:n_eig].max())})
    fl.close()
    fc.close()


if __name__ == "__main__":
    main()
