#!/usr/bin/env python3
"""Time the direct solver on the LOD space next to the CG it replaces, on BASELINE configuration C2 (2-D Poisson,
H = 1/32, n_sub 8, oversampling 2: 1024 unknowns, half bandwidth 165, D1e4 coefficient), all in one run:

  factor      slod_lod_factor_create of the symmetrised A_LOD (64 queued launches and the read-back of the pivots)
  solve       slod_lod_factor_solve for n_rhs = 1, 16, 64 next to slod_lod_solve_multi at rel_tol = 1e-12 on the same
              matrix and loads f_k = sin(k pi x) sin(pi y)
  steps       slod_lod_theta_steps_direct (Crank-Nicolson) and slod_lod_newmark_steps_direct (trapezoidal rule, with
              energies) next to slod_lod_theta_steps / slod_lod_newmark_steps at rel_tol = 1e-12, 8 steps per call,
              dt = 0.7 / omega_1 (omega_1 from slod_lod_eigs), n_rhs = 1, 16, 64; the factor of S is made outside the
              timed call and timed on its own
  break_even  the number of steps after which factor + direct steps undercut the CG loop: factor_ms / (cg - direct)

HIP-event time of each call (median of --reps after a warm-up; for the synchronising calls the events enclose the
allocation of the call's workspace and its synchronisations).  One JSON line per measurement; nothing is asserted.

  python tools/lod_direct_timing.py [--reps 5]
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
REL_TOL = 1e-12
STEPS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_direct_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    values, mvalues, S = torch.zeros_like(raw), torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mvalues.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), values.data_ptr())
    torch.cuda.synchronize()
    X = torch.zeros(NP, 5, dtype=torch.float64, device=dev)
    lam, _, _ = g.lod_eigs(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), 1, X.data_ptr(), n_block=5)
    dt = 0.7 / math.sqrt(lam[0])

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

    def factor_of(vals):
        made = []

        def run():
            while made:
                made.pop().close()
            made.append(g.lod_factor(vals.data_ptr(), cols.data_ptr()))
        tt = median(run)
        return made[0], tt

    fA, tt = factor_of(values)
    info = fA.info
    print(json.dumps({"factor_event_ms": tt[0], "factor_wall_ms": tt[1], "n": info.n, "half_bandwidth": info.half_bandwidth,
                      "block": info.block, "bytes": info.bytes, "min_pivot": info.min_pivot, "max_pivot": info.max_pivot,
                      "dt": dt}), flush=True)

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

    # the factors of the two time loops, timed like the first
    g.lod_matrix_combine(1.0, mvalues.data_ptr(), 0.5 * dt, values.data_ptr(), S.data_ptr())
    torch.cuda.synchronize()
    f_cn, t_cn = factor_of(S)
    S2 = torch.zeros_like(S)
    g.lod_matrix_combine(1.0, mvalues.data_ptr(), 0.25 * dt * dt, values.data_ptr(), S2.data_ptr())
    torch.cuda.synchronize()
    f_tr, t_tr = factor_of(S2)
    fM = g.lod_factor(mvalues.data_ptr(), cols.data_ptr())

    for nr in (1, 16, 64):
        B = Ball[:, :nr].contiguous()
        U, Ud, V, A, A0 = (torch.zeros_like(B) for _ in range(5))
        rec = {"n_rhs": nr, "steps": STEPS}
        # asynchronous: on torch's stream, where the events are recorded
        tt = median(lambda: fA.solve(B.data_ptr(), Ud.data_ptr(), n_rhs=nr, stream=torch.cuda.current_stream().cuda_stream))
        rec["factor_solve_event_ms"], rec["factor_solve_wall_ms"] = tt
        cg = lambda: g.lod_solve_multi(values.data_ptr(), cols.data_ptr(), B.data_ptr(), nr, nr, U.data_ptr(), nr, REL_TOL, 20000)
        tt = median(cg)
        rec["cg_solve_event_ms"], rec["cg_solve_wall_ms"] = tt
        rec["cg_solve_iterations"] = int(cg()[0].max())
        rec["solve_max_rel_difference"] = float(((U - Ud).abs().max() / U.abs().max()).item())
        g.lod_newmark_accel_direct(fM, values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), U.data_ptr(), V.data_ptr(),
                                   A0.data_ptr(), n_rhs=nr, d_load=B.data_ptr())

        def theta(direct):
            def run():
                U.zero_()
                if direct:
                    return g.lod_theta_steps_direct(f_cn, values.data_ptr(), cols.data_ptr(), dt, 0.5, STEPS, U.data_ptr(), n_rhs=nr,
                                                    d_load=B.data_ptr())
                return g.lod_theta_steps(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), dt, 0.5, STEPS, U.data_ptr(),
                                         n_rhs=nr, d_load=B.data_ptr(), rel_tol=REL_TOL, max_iterations=20000)
            return run

        def newmark(direct):
            def run():
                U.zero_()
                V.zero_()
                A.copy_(A0)
                if direct:
                    return g.lod_newmark_steps_direct(f_tr, values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), dt, STEPS,
                                                      U.data_ptr(), V.data_ptr(), A.data_ptr(), n_rhs=nr, d_load=B.data_ptr())
                return g.lod_newmark_steps(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), dt, STEPS, U.data_ptr(),
                                           V.data_ptr(), A.data_ptr(), n_rhs=nr, d_load=B.data_ptr(), rel_tol=REL_TOL,
                                           max_iterations=20000)
            return run

        for key, make, fac in (("crank_nicolson", theta, t_cn), ("trapezoidal", newmark, t_tr)):
            td, tc = median(make(True)), median(make(False))
            rec[key + "_direct_event_ms_per_step"] = td[0] / STEPS
            rec[key + "_cg_event_ms_per_step"] = tc[0] / STEPS
            rec[key + "_cg_iterations_per_step"] = make(False)()[0].tolist()
            rec[key + "_factor_event_ms"] = fac[0]
            gain = (tc[0] - td[0]) / STEPS
            rec[key + "_break_even_steps"] = math.ceil(fac[0] / gain) if gain > 0 else None
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
