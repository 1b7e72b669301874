#!/usr/bin/env python3
"""Time the two-stage implicit Runge-Kutta steppers on the LOD space on BASELINE configuration C2 (2-D Poisson, H = 1/32,
n_sub 8, oversampling 2: 1024 patches = 1024 rows, half bandwidth 165, D1e4 coefficient) for 1 and 16 columns.

  step      ms per step of slod_lod_irk_heat_steps_direct and slod_lod_irk_wave_steps_direct, Gauss and Radau, the wave
            with and without energies: one call of --steps steps (queued whole, waited for once) divided by --steps
  yardstick the same of slod_lod_theta_steps_direct (theta = 1/2) and slod_lod_newmark_steps_direct (beta = 1/4) on their
            real Cholesky factors, what the library offered before
  factor    slod_lod_factor_create_zldl on the pair of slod_lod_irk_coefficients against slod_lod_factor_create_ldl and
            slod_lod_factor_create on the real step matrix (with their destroy), and the bytes each owns
  launches  per step, counted from the loops: 3 (right-hand side, complex solve, update), 5 with energies; the theta and
            Newmark loops on a factor 4, 6 with energies
  steps     what each scheme needs for a relative error of 1e-4 and 1e-6 in the lowest wave mode over ten periods, from
            the 2 x 2 amplification matrix on the CPU (Pade (2,2) for Gauss, (1,2) for Radau, (1,1) for the trapezoidal
            rule), times the measured ms per step without energies
dt = 0.5 / sqrt(lambda_1) (lambda from slod_lod_eigs_direct); the time of a step does not depend on it.
Wall-clock times around a device synchronisation: minimum, median and maximum of --reps runs after a warm-up.  No time
and no ratio is asserted anywhere.  One JSON line per measurement, printed and, with --out, appended to that file.

  python tools/lod_irk_timing.py [--reps 7] [--steps 8] [--out profiles/lod_irk_timing.txt]
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
SCHEMES = ("gauss", "radau")


def amplification(scheme, x):
    """R(x) of the 2 x 2 matrix x: Pade (2,2), (1,2) or (1,1) of exp."""
    I = np.eye(2)
    if scheme == "gauss":
        return np.linalg.solve(I - x / 2.0 + x @ x / 12.0, I + x / 2.0 + x @ x / 12.0)
    if scheme == "radau":
        return np.linalg.solve(I - 2.0 * x / 3.0 + x @ x / 6.0, I + x / 3.0)
    return np.linalg.solve(I - x / 2.0, I + x / 2.0)


def steps_needed(scheme, tol, periods=10):
    """The fewest steps over `periods` periods of u'' + u = 0 from (1, 0) with |(u, u') - exact| <= tol at the end."""
    def err(n):
        dt = 2.0 * np.pi * periods / n
        y = np.linalg.matrix_power(amplification(scheme, dt * np.array([[0.0, 1.0], [-1.0, 0.0]])), n) @ np.array([1.0, 0.0])
        return float(np.abs(y - np.array([1.0, 0.0])).max())
    lo, hi = periods, 4 * periods
    while err(hi) > tol:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:                     # the error falls monotonically once the step resolves the period
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if err(mid) <= tol else (mid, hi)
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_irk_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    sym, mass, S = torch.zeros_like(raw), torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mass.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), sym.data_ptr())
    torch.cuda.synchronize()
    A, M, Cc = sym.data_ptr(), mass.data_ptr(), cols.data_ptr()

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def stats(fn, per=1):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / per)
        ms.sort()
        return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

    fc = g.lod_factor(A, Cc)
    X = torch.zeros(nrow, 16, dtype=torch.float64, device=dev)
    low = g.lod_eigs_direct(fc, A, M, Cc, 8, X.data_ptr(), n_block=16, ld_x=16)[0]
    fc.close()
    w1 = float(np.sqrt(low[0]))
    dt, K = 0.5 / w1, args.steps
    emit({"rows": nrow, "lambda_1": float(low[0]), "dt": dt, "steps_per_call": K, "reps": args.reps,
          "launches_per_step": {"irk": 3, "irk_with_energies": 5, "theta_direct": 4, "newmark_direct": 4,
                                "newmark_direct_with_energies": 6}})

    # the factors
    g.lod_matrix_combine(1.0, M, 0.25 * dt * dt, A, S.data_ptr())
    torch.cuda.synchronize()
    pair = g.lod_irk_coefficients("gauss", 2, dt)
    t_z = stats(lambda: g.lod_factor_zldl(A, M, Cc, [pair[0]], [pair[1]]).close())
    t_l = stats(lambda: g.lod_factor_ldl(S.data_ptr(), Cc).close())
    t_c = stats(lambda: g.lod_factor(S.data_ptr(), Cc).close())
    fz = g.lod_factor_zldl(A, M, Cc, [pair[0]], [pair[1]])
    fl = g.lod_factor_ldl(S.data_ptr(), Cc)
    emit({"factor": "gauss wave step matrix", "create_zldl_ms": t_z, "create_ldl_ms": t_l, "create_cholesky_ms": t_c,
          "zldl_over_ldl_median": t_z["median"] / t_l["median"], "complex_factor_bytes": int(fz.info.bytes),
          "real_factor_bytes": int(fl.info.bytes), "growth": fz.inertia(0).growth})
    fz.close()
    fl.close()

    per_step = {}
    for n in (1, 16):
        rng = np.random.default_rng(7)
        u0 = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
        load = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
        U, V, Acc = torch.zeros_like(u0), torch.zeros_like(u0), torch.zeros_like(u0)

        def reset():
            U.copy_(u0)
            V.zero_()
            Acc.zero_()

        # the yardsticks on their real factors
        g.lod_matrix_combine(1.0, M, 0.5 * dt, A, S.data_ptr())
        torch.cuda.synchronize()
        fS = g.lod_factor(S.data_ptr(), Cc)
        reset()
        t_theta = stats(lambda: g.lod_theta_steps_direct(fS, A, Cc, dt, 0.5, K, U.data_ptr(), n_rhs=n, d_load=load.data_ptr()), K)
        fS.close()
        g.lod_matrix_combine(1.0, M, 0.25 * dt * dt, A, S.data_ptr())
        torch.cuda.synchronize()
        fS = g.lod_factor(S.data_ptr(), Cc)
        t_nm = {}
        for energies in (False, True):
            reset()
            t_nm[energies] = stats(lambda: g.lod_newmark_steps_direct(fS, A, M, Cc, dt, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr(),
                                                                      n_rhs=n, d_load=load.data_ptr(), energies=energies), K)
        fS.close()
        emit({"n_rhs": n, "yardstick": True, "theta_direct_ms_per_step": t_theta, "newmark_direct_ms_per_step": t_nm[False],
              "newmark_direct_with_energies_ms_per_step": t_nm[True]})
        per_step["trapezoidal", n] = t_nm[False]["median"]
        for scheme in SCHEMES:
            ah, bh = g.lod_irk_coefficients(scheme, 1, dt)
            aw, bw = g.lod_irk_coefficients(scheme, 2, dt)
            f = g.lod_factor_zldl(A, M, Cc, [ah, aw], [bh, bw])
            reset()
            t_heat = stats(lambda: g.lod_irk_heat_steps(f, scheme, A, Cc, dt, K, U.data_ptr(), n_rhs=n, member=0,
                                                        d_load=load.data_ptr()), K)
            t_wave = {}
            for energies in (False, True):
                reset()
                t_wave[energies] = stats(lambda: g.lod_irk_wave_steps(f, scheme, A, M, Cc, dt, K, U.data_ptr(), V.data_ptr(), n_rhs=n,
                                                                      member=1, d_load=load.data_ptr(), energies=energies), K)
            f.close()
            per_step[scheme, n] = t_wave[False]["median"]
            emit({"n_rhs": n, "scheme": scheme, "heat_ms_per_step": t_heat, "wave_ms_per_step": t_wave[False],
                  "wave_with_energies_ms_per_step": t_wave[True],
                  "heat_over_theta_median": t_heat["median"] / t_theta["median"],
                  "wave_over_newmark_median": t_wave[False]["median"] / t_nm[False]["median"],
                  "wave_with_energies_over_newmark_median": t_wave[True]["median"] / t_nm[True]["median"]})

    # the price of an accuracy: steps from the CPU, times the measured step
    for tol in (1e-4, 1e-6):
        need = {s: steps_needed(s, tol) for s in ("gauss", "radau", "trapezoidal")}
        emit({"lowest_wave_mode_over_ten_periods_rel_error": tol, "steps": need,
              "ms": {"%s, %d columns" % (s, n): need[s] * per_step[s, n] for s in need for n in (1, 16)}})


if __name__ == "__main__":
    main()
