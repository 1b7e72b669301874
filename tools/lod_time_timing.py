#!/usr/bin/env python3
"""Time slod_lod_mass_matrix next to slod_lod_matrix, and a step of slod_lod_theta_steps next to one
slod_lod_solve_multi call, on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8, oversampling 2: 1024
patches, 49 slots per block row, D1e4 coefficient).

Matrix kernels, in the same run: HIP-event time of each call for all 1024 rows (median of --reps after a warm-up; the
events enclose the upload of the row list and the synchronisation the call does), and the bytes each must move at
least once: every used slot reads the overlap rectangle of the two slabs it pairs (phi of the row patch and psi, for
the mass phi, of the column patch; 8 bytes per node each) and writes one value and one column.  The rate that implies
is a lower bound of the traffic, since the corner loads of the mass kernel touch every node up to four times (from
cache).

Stepper: backward Euler, dt = 1e-3, 8 steps per call, rel_tol 1e-10, loads f_k = sin(k pi x) sin(pi y) constant in
time, u^0 = 0, for n_rhs in 1, 16, 64: event time per step, iterations per step; next to it one slod_lod_solve_multi
call on the elliptic system with the same loads and tolerance.  One JSON line per measurement.

  python tools/lod_time_timing.py [--reps 5]
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
REL_TOL = 1e-10
DT, STEPS = 1e-3, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_time_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    NP, cap, n = g.num_patches, g.lod_row_capacity(), C2["n_sub"]
    values = torch.zeros(NP * cap, dtype=torch.float64, device=dev)
    mvalues = torch.zeros_like(values)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)

    def timed(fn):
        """(event ms, wall ms, result) of fn(); the events sit on the null stream around a synchronising call."""
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

    def stiffness():
        g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, values.data_ptr(), cols.data_ptr())

    def mass():
        g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mvalues.data_ptr(), mcols.data_ptr())

    ts, tm = median(stiffness), median(mass)
    hc = cols.cpu().numpy().view(np.uint32).reshape(NP, cap)
    assert np.array_equal(hc.ravel(), mcols.cpu().numpy().view(np.uint32))
    info = [g.patch_layout(p) for p in range(NP)]
    nodes = elements = 0
    for p in range(NP):
        for c in hc[p][hc[p] != 0xffffffff]:
            a, o = info[p], info[int(c)]
            w = (min(a.x0 + a.mx, o.x0 + o.mx) - max(a.x0, o.x0)) * n
            hgt = (min(a.y0 + a.my, o.y0 + o.my) - max(a.y0, o.y0)) * n
            nodes += (w + 1) * (hgt + 1)
            elements += w * hgt
    used = int((hc != 0xffffffff).sum())
    pair_bytes = nodes * 2 * 8 + NP * cap * 12
    for name, tt in (("slod_lod_matrix", ts), ("slod_lod_mass_matrix", tm)):
        print(json.dumps({"call": name, "rows": NP, "used_slots": used, "overlap_nodes": nodes, "overlap_elements": elements,
                          "event_ms": tt[0], "wall_ms": tt[1], "compulsory_bytes": pair_bytes,
                          "GBps_lower_bound": pair_bytes / (tt[0] * 1e-3) / 1e9}), flush=True)
    print(json.dumps({"mass_over_stiffness_event_time": tm[0] / ts[0]}), flush=True)

    # loads for the stepper and the elliptic solve
    kmax = 64
    g0 = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
    ey, ex, qq = np.meshgrid(np.arange(g.NE), np.arange(g.NE), np.arange(4), indexing="ij")
    x = ((ex + np.where(qq & 1, 1.0 - g0, g0)) / g.NE).ravel()
    y = ((ey + np.where(qq & 2, 1.0 - g0, g0)) / g.NE).ravel()
    nfine = (g.NE + 1) ** 2
    F = torch.zeros(kmax, nfine, dtype=torch.float64, device=dev)
    for k in range(kmax):
        fq = torch.from_numpy(np.sin((k + 1) * np.pi * x) * np.sin(np.pi * y)).to(dev)
        g.fem_rhs(fq.data_ptr(), F[k].data_ptr())
        torch.cuda.synchronize()
    Ball = torch.zeros(NP, kmax, dtype=torch.float64, device=dev)
    g.lod_rhs_multi(ids, b.data_ptr(), plan.stride, F.data_ptr(), nfine, kmax, Ball.data_ptr(), kmax)
    for nr in (1, 16, 64):
        B = Ball[:, :nr].contiguous()
        U = torch.zeros_like(B)

        def steps():
            U.zero_()
            return g.lod_theta_steps(values.data_ptr(), mvalues.data_ptr(), cols.data_ptr(), DT, 1.0, STEPS, U.data_ptr(),
                                     n_rhs=nr, d_load=B.data_ptr(), rel_tol=REL_TOL, max_iterations=20000)

        def elliptic():
            return g.lod_solve_multi(values.data_ptr(), cols.data_ptr(), B.data_ptr(), nr, nr, U.data_ptr(), nr, REL_TOL, 20000)

        tstep, tell = median(steps), median(elliptic)
        its, res = steps()
        eit, eres = elliptic()
        print(json.dumps({"n_rhs": nr, "steps": STEPS, "dt": DT, "theta": 1.0, "steps_event_ms": tstep[0],
                          "steps_wall_ms": tstep[1], "event_ms_per_step": tstep[0] / STEPS,
                          "iterations_per_step": its.tolist(), "max_rel_residual": float(res.max()),
                          "elliptic_event_ms": tell[0], "elliptic_wall_ms": tell[1],
                          "elliptic_iterations_max": int(eit.max()), "elliptic_max_rel_residual": float(eres.max())}),
              flush=True)


if __name__ == "__main__":
    main()
