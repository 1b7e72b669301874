#!/usr/bin/env python3
"""Time the frequency response on the LOD space on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8,
oversampling 2: 1024 patches = 1024 rows, half bandwidth 165, D1e4 coefficient) for K = 1, 8, 64 frequencies and 1 and 16
load columns.  The frequencies are evenly spaced in [sqrt(lambda_1) / 2, 2 sqrt(lambda_8)] (K = 1: 1.5 sqrt(lambda_1); lambda from
slod_lod_eigs_direct), the damping is dm = 0.02 sqrt(lambda_1), ds = 1e-3 / sqrt(lambda_1).

  sweep     slod_lod_harmonic_response, the whole call
  factor    slod_lod_factor_create_zldl on the K pairs (alpha, beta) of the sweep (and its destroy)
  solve     slod_lod_factor_solve_complex on that factor, the load shared by the members
  residual  sweep - factor - solve: the four products, the residual kernels and the read-back of the norms
  baseline  K sequential slod_lod_matrix_combine + slod_lod_factor_create_ldl + slod_lod_factor_solve on
            sym(A) - omega^2 M, the only thing the library offered before: undamped, one real factor per call
Wall-clock times around a device synchronisation (the create calls wait for their read-back themselves): minimum, median
and maximum of --reps runs after a warm-up, with the bytes a factor owns.  No time and no ratio is asserted anywhere: the
complex factor does four times the matrix-pipe work of the real one and moves twice the words.  One JSON line per
measurement, printed and, with --out, appended to that file.

  python tools/lod_harmonic_timing.py [--reps 7] [--out profiles/lod_harmonic_timing.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_harmonic_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    sym, mass, shifted = torch.zeros_like(raw), torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mass.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), sym.data_ptr())
    torch.cuda.synchronize()

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def stats(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

    fc = g.lod_factor(sym.data_ptr(), cols.data_ptr())
    X = torch.zeros(nrow, 16, dtype=torch.float64, device=dev)
    low = g.lod_eigs_direct(fc, sym.data_ptr(), mass.data_ptr(), cols.data_ptr(), 8, X.data_ptr(), n_block=16, ld_x=16)[0]
    fc.close()
    w_lo, w_hi = 0.5 * float(np.sqrt(low[0])), 2.0 * float(np.sqrt(low[7]))
    dm, ds = 0.02 * float(np.sqrt(low[0])), 1e-3 / float(np.sqrt(low[0]))
    emit({"rows": nrow, "lambda_1": float(low[0]), "lambda_8": float(low[7]), "omega_range": [w_lo, w_hi], "damp_mass": dm,
          "damp_stiff": ds, "reps": args.reps})

    for K in (1, 8, 64):
        omegas = np.linspace(w_lo, w_hi, K) if K > 1 else np.array([1.5 * float(np.sqrt(low[0]))])
        alpha, beta = 1.0 + 1j * (omegas * ds), -(omegas * omegas) + 1j * (omegas * dm)
        for n in (1, 16):
            B = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 1.0, (nrow, n))).to(dev)
            ur, ui = torch.zeros(nrow, K * n, dtype=torch.float64, device=dev), torch.zeros(nrow, K * n, dtype=torch.float64, device=dev)
            xr = torch.zeros(nrow, n, dtype=torch.float64, device=dev)
            out = {}

            def sweep():
                out["res"], out["growth"] = g.lod_harmonic_response(sym.data_ptr(), mass.data_ptr(), cols.data_ptr(), omegas, B.data_ptr(),
                                                                    None, ur.data_ptr(), ui.data_ptr(), n_rhs=n, damp_mass=dm,
                                                                    damp_stiff=ds)

            def factor():
                g.lod_factor_zldl(sym.data_ptr(), mass.data_ptr(), cols.data_ptr(), alpha, beta).close()

            def baseline():
                for w in omegas:
                    g.lod_matrix_combine(1.0, sym.data_ptr(), -(w * w), mass.data_ptr(), shifted.data_ptr())
                    f = g.lod_factor_ldl(shifted.data_ptr(), cols.data_ptr())
                    f.solve(B.data_ptr(), xr.data_ptr(), n_rhs=n)
                    f.close()

            t_sweep, t_factor = stats(sweep), stats(factor)
            fz = g.lod_factor_zldl(sym.data_ptr(), mass.data_ptr(), cols.data_ptr(), alpha, beta)
            t_solve = stats(lambda: fz.solve_complex(B.data_ptr(), None, ur.data_ptr(), ui.data_ptr(), n_rhs=n, shared_rhs=True))
            zbytes = int(fz.info.bytes)
            fz.close()
            t_base = stats(baseline)
            g.lod_matrix_combine(1.0, sym.data_ptr(), -(omegas[0] ** 2), mass.data_ptr(), shifted.data_ptr())
            fr = g.lod_factor_ldl(shifted.data_ptr(), cols.data_ptr())
            rbytes, rgrowth = int(fr.info.bytes), fr.inertia().growth
            fr.close()
            emit({"n_freq": K, "n_rhs": n, "sweep_ms": t_sweep, "factor_ms": t_factor, "solve_ms": t_solve,
                  "residual_ms_median": t_sweep["median"] - t_factor["median"] - t_solve["median"], "baseline_ms": t_base,
                  "sweep_over_baseline_median": t_sweep["median"] / t_base["median"],
                  "complex_factor_bytes": zbytes, "complex_factor_bytes_per_frequency": zbytes // K, "real_factor_bytes": rbytes,
                  "max_rel_residual": float(out["res"].max()), "max_growth": float(out["growth"].max()),
                  "undamped_real_growth_at_first_omega": rgrowth})


if __name__ == "__main__":
    main()
