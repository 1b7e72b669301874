#!/usr/bin/env python3
"""Time one step of slod_lod_newmark_steps next to one step of slod_lod_theta_steps on BASELINE configuration C2 (2-D
Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 patches, 49 slots per block row, D1e4 coefficient), with and without
the energy kernel.

Both steppers run 8 steps per call at rel_tol 1e-10 from rest with the loads f_k = sin(k pi x) sin(pi y), constant in
time, for n_rhs in 1, 16, 64; the stiffness is symmetrised for both.  The time step is the same for both, 0.7 / omega_1
with omega_1 from slod_lod_eigs: the trapezoidal rule (beta = 1/4) then solves with M + dt^2 / 4 A, Crank-Nicolson
(theta = 1/2) with M + dt / 2 A, so the iteration counts differ and are printed next to the times.  Central differences
(beta = 0) run at 1.8 / omega_max, omega_max from a few power iterations on the host copy of the pencil, and solve with
a multiple of M.  HIP-event time of each call (median of --reps after a warm-up; the events enclose the allocation of
the call's workspace and its synchronisations).  One JSON line per measurement; nothing is asserted.

  python tools/lod_wave_timing.py [--reps 5]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-slod_amd"))

SEED = 20250614
C2 = dict(nref=5, n_sub=8, oversampling=2, spacedim=1, stabilize=1)
REL_TOL = 1e-10
STEPS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_wave_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    raw = torch.zeros(NP * cap, dtype=torch.float64, device=dev)
    values, mvalues = torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mvalues.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), values.data_ptr())
    torch.cuda.synchronize()

    # omega_1 on the device; omega_max by power iteration on M^-1 A with the library's product and mass solve
    X = torch.zeros(NP, 5, dtype=torch.float64, device=dev)
    lam, _, _ = g.lod_eigs(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), 1, X.data_ptr(), n_block=5)
    w1 = math.sqrt(lam[0])
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, NP)).to(dev)
    y, z = torch.zeros_like(x), torch.zeros_like(x)
    top = 0.0
    for _ in range(60):
        g.lod_apply(values.data_ptr(), cols.data_ptr(), x.data_ptr(), y.data_ptr())
        g.lod_solve_multi(mvalues.data_ptr(), cols.data_ptr(), y.data_ptr(), 1, 1, z.data_ptr(), 1, 1e-10, 2000)
        top = float(torch.linalg.norm(z) / torch.linalg.norm(x))
        x = z / torch.linalg.norm(z)
    # 60 iterations approach lambda_max from below; the explicit run keeps the margin 1.8 < 2
    wmax = math.sqrt(top)
    print(json.dumps({"omega_1": w1, "omega_max_power_iteration": wmax}), flush=True)

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

    kmax = 64
    g0 = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
    ey, ex, qq = np.meshgrid(np.arange(g.NE), np.arange(g.NE), np.arange(4), indexing="ij")
    xs = ((ex + np.where(qq & 1, 1.0 - g0, g0)) / g.NE).ravel()
    ys = ((ey + np.where(qq & 2, 1.0 - g0, g0)) / g.NE).ravel()
    nfine = (g.NE + 1) ** 2
    F = torch.zeros(kmax, nfine, dtype=torch.float64, device=dev)
    for k in range(kmax):
        fq = torch.from_numpy(np.sin((k + 1) * np.pi * xs) * np.sin(np.pi * ys)).to(dev)
        g.fem_rhs(fq.data_ptr(), F[k].data_ptr())
        torch.cuda.synchronize()
    Ball = torch.zeros(NP, kmax, dtype=torch.float64, device=dev)
    g.lod_rhs_multi(ids, b.data_ptr(), plan.stride, F.data_ptr(), nfine, kmax, Ball.data_ptr(), kmax)
    for nr in (1, 16, 64):
        B = Ball[:, :nr].contiguous()
        U, V, A, A0 = (torch.zeros_like(B) for _ in range(4))
        g.lod_newmark_accel(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), U.data_ptr(), V.data_ptr(), A0.data_ptr(),
                            n_rhs=nr, d_load=B.data_ptr(), rel_tol=REL_TOL, max_iterations=20000)

        def newmark(dt, beta, energies):
            def run():
                U.zero_()
                V.zero_()
                A.copy_(A0)
                return g.lod_newmark_steps(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), dt, STEPS, U.data_ptr(),
                                           V.data_ptr(), A.data_ptr(), beta=beta, n_rhs=nr, d_load=B.data_ptr(),
                                           rel_tol=REL_TOL, max_iterations=20000, energies=energies)
            return run

        def theta(dt):
            def run():
                U.zero_()
                return g.lod_theta_steps(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), dt, 0.5, STEPS, U.data_ptr(),
                                         n_rhs=nr, d_load=B.data_ptr(), rel_tol=REL_TOL, max_iterations=20000)
            return run

        dt_i, dt_e = 0.7 / w1, 1.8 / wmax
        rec = {"n_rhs": nr, "steps": STEPS, "dt_implicit": dt_i, "dt_explicit": dt_e}
        for key, fn in (("trapezoidal_energies", newmark(dt_i, 0.25, True)), ("trapezoidal", newmark(dt_i, 0.25, False)),
                        ("central_energies", newmark(dt_e, 0.0, True)), ("central", newmark(dt_e, 0.0, False)),
                        ("crank_nicolson", theta(dt_i))):
            tt = median(fn)
            out = fn()
            rec[key + "_event_ms_per_step"] = tt[0] / STEPS
            rec[key + "_wall_ms_per_step"] = tt[1] / STEPS
            rec[key + "_iterations_per_step"] = out[0].tolist()
            rec[key + "_max_rel_residual"] = float(out[1].max())
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
