#!/usr/bin/env python3
"""Time the ensemble factor next to what it replaces, on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8,
oversampling 2: 1024 unknowns per member, half bandwidth 165), K members with D1e4 coefficients of their own (seeds
SEED + k), all in one run and for every K of --members:

  factor   slod_lod_factor_create_ensemble of S = M + dt/2 sym(A) next to K sequential slod_lod_factor_create on the
           de-interleaved members
  solve    slod_lod_factor_solve_ensemble (n_rhs = 1 per member) next to K sequential slod_lod_factor_solve(n_rhs = 1)
  step     a Crank-Nicolson step of all members: slod_lod_theta_steps_ensemble_direct (STEPS steps per call, per step)
           next to slod_lod_solve_ensemble at rel_tol = 1e-12 on the same S (the solve of one CG step for all members)
           and next to K sequential slod_lod_theta_steps_direct
dt = 0.7 / omega_1 of member 0 (slod_lod_eigs), as tools/lod_direct_timing.py.

HIP-event time of each call (median of --reps after a warm-up, with the least and the largest in event_ms_range; the
events sit on the null stream and the calls end synchronised, so for the synchronising calls they enclose the allocation
of the workspace and the waits).  One JSON line per K; nothing is asserted.

  python tools/lod_ensemble_direct_timing.py [--reps 5] [--members 1 8 64]
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
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64])
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_ensemble_direct_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    kmax = max(args.members)
    g = slod_amd.Slod(n_problems=kmax, **C2)
    for k in range(kmax):
        t = torch.from_numpy(fill_coefficient(SEED + k, "D1e4", g.NE)).to(dev)
        g.set_coefficient_device(0, t.data_ptr(), t.numel(), problem=k)
        torch.cuda.synchronize()
    NP, cap = g.num_patches, g.lod_row_capacity()
    plan = g.plan(np.arange(kmax * NP, dtype=np.uint32))
    stride = plan.stride
    b = torch.zeros(kmax * NP * stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    nfine, nval = (g.NE + 1) ** 2, NP * cap
    load = torch.zeros(nfine, dtype=torch.float64, device=dev)
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        torch.cuda.synchronize()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def median(fn):
        """(median event ms, median wall ms, [least, largest event ms]) of --reps runs after a warm-up"""
        fn()
        runs = sorted(timed(fn) for _ in range(args.reps))
        return runs[args.reps // 2] + ([runs[0][0], runs[-1][0]],)

    dt = None
    for K in args.members:
        raw, A, M, S = (torch.zeros(nval, K, dtype=torch.float64, device=dev) for _ in range(4))
        cols = torch.zeros(nval, dtype=torch.int32, device=dev)
        mcols = torch.zeros_like(cols)
        R = torch.zeros(NP, K, dtype=torch.float64, device=dev)
        g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), stride, K, raw.data_ptr(), cols.data_ptr())
        g.lod_mass_matrix_ensemble(b.data_ptr(), stride, K, M.data_ptr(), mcols.data_ptr())
        g.lod_matrix_symmetrize_ensemble(raw.data_ptr(), cols.data_ptr(), K, A.data_ptr())
        g.lod_rhs_ensemble(b.data_ptr(), stride, K, load.data_ptr(), R.data_ptr())
        torch.cuda.synchronize()
        if dt is None:                                                        # member 0 is the same for every K
            X = torch.zeros(NP, 5, dtype=torch.float64, device=dev)
            lam, _, _ = g.lod_eigs(A[:, 0].contiguous().data_ptr(), M[:, 0].contiguous().data_ptr(), cols.data_ptr(), 1,
                                   X.data_ptr(), n_block=5)
            dt = 0.7 / math.sqrt(lam[0])
        g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), 0.5 * dt, A.data_ptr(), K, S.data_ptr())
        torch.cuda.synchronize()
        Ak = [A[:, k].contiguous() for k in range(K)]
        Sk = [S[:, k].contiguous() for k in range(K)]
        Rk = [R[:, k].contiguous() for k in range(K)]
        U, D = torch.zeros_like(R), torch.zeros_like(R)
        u1 = torch.zeros(NP, dtype=torch.float64, device=dev)
        made, singles, out = [], [], {}

        def factor_ens():
            while made:
                made.pop().close()
            made.append(g.lod_factor_ensemble(S.data_ptr(), cols.data_ptr(), K))

        def factor_seq():
            while singles:
                singles.pop().close()
            for k in range(K):
                singles.append(g.lod_factor(Sk[k].data_ptr(), cols.data_ptr()))

        tfe, tfs = median(factor_ens), median(factor_seq)
        f = made[0]
        st = torch.cuda.current_stream().cuda_stream

        def solve_ens():
            f.solve(R.data_ptr(), D.data_ptr(), stream=st)

        def solve_seq():
            for k in range(K):
                singles[k].solve(Rk[k].data_ptr(), u1.data_ptr(), stream=st)

        tse, tss = median(solve_ens), median(solve_seq)

        def step_ens():
            U.zero_()
            g.lod_theta_steps_ensemble_direct(f, A.data_ptr(), cols.data_ptr(), dt, 0.5, STEPS, K, U.data_ptr(), d_load=R.data_ptr())

        def step_seq():
            for k in range(K):
                u1.zero_()
                g.lod_theta_steps_direct(singles[k], Ak[k].data_ptr(), cols.data_ptr(), dt, 0.5, STEPS, u1.data_ptr(),
                                         d_load=Rk[k].data_ptr())

        def step_cg():
            out["cg"] = g.lod_solve_ensemble(S.data_ptr(), cols.data_ptr(), R.data_ptr(), D.data_ptr(), K, rel_tol=REL_TOL,
                                             max_iterations=20000)

        tte, tts, ttc = median(step_ens), median(step_seq), median(step_cg)
        print(json.dumps({
            "n_members": K, "dt": dt, "steps_per_call": STEPS, "n": f.info.n, "half_bandwidth": f.info.half_bandwidth,
            "factor_bytes": f.info.bytes, "factor_bytes_per_member": f.info.bytes // K,
            "min_pivot": f.info.min_pivot, "max_pivot": f.info.max_pivot,
            "factor_ensemble_event_ms": tfe[0], "factor_ensemble_wall_ms": tfe[1],
            "factor_sequential_event_ms": tfs[0], "factor_sequential_wall_ms": tfs[1], "factor_speedup_event": tfs[0] / tfe[0],
            "solve_ensemble_event_ms": tse[0], "solve_ensemble_wall_ms": tse[1],
            "solve_sequential_event_ms": tss[0], "solve_sequential_wall_ms": tss[1], "solve_speedup_event": tss[0] / tse[0],
            "cn_step_ensemble_direct_event_ms": tte[0] / STEPS, "cn_step_sequential_direct_event_ms": tts[0] / STEPS,
            "cn_step_cg_ensemble_solve_event_ms": ttc[0], "cn_step_cg_iterations_max": int(out["cg"][0].max()),
            "cn_step_speedup_over_sequential": tts[0] / tte[0], "cn_step_speedup_over_cg": ttc[0] * STEPS / tte[0],
            "event_ms_range": {"factor_ensemble": tfe[2], "factor_sequential": tfs[2], "solve_ensemble": tse[2],
                               "solve_sequential": tss[2], "cn_call_ensemble_direct": tte[2], "cn_call_sequential_direct": tts[2],
                               "cn_cg_ensemble_solve": ttc[2]}}), flush=True)
        for x in made + singles:
            x.close()


if __name__ == "__main__":
    main()
