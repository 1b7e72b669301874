#!/usr/bin/env python3
"""Time slod_lod_solve_multi against n_rhs back-to-back slod_lod_solve calls on BASELINE configuration C2
(2-D Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 patches, 49 slots per block row), rel_tol 1e-10.

For n_rhs in 1, 4, 16, 64, 256: HIP-event and host wall time of one multi-vector solve (median of --reps after a
warm-up), the same for n_rhs single-vector solves of the same loads, iterations, launches per iteration (counted
from the algorithm: 3 per iteration + 1 check per burst of 8 for the multi-vector solve, 4 per iteration for the
single-vector one), and the bytes the matrix product must move per iteration (values, cols, P read once per slot,
Y written) over the event time of the whole solve: a lower bound of the product's rate, since the solve also runs
the two update kernels.  Loads: f_k = sin(k pi x) sin(pi y), k = 1 .. n_rhs.  One JSON line per n_rhs.

  python tools/lod_multi_timing.py [--reps 5] [--only-multi N]     (--only-multi: one solve, for a profiler run)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-multi", type=int, default=0, metavar="N")
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_multi_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    values = torch.zeros(NP * cap, dtype=torch.float64, device=dev)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, values.data_ptr(), cols.data_ptr())
    used = int((cols.cpu().numpy().view(np.uint32) != 0xffffffff).sum())
    # loads at the quadrature points, fine load vectors, C^T F for the widest case
    kmax = max(256, args.only_multi)
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

    if args.only_multi:
        n = args.only_multi
        B = Ball[:, :n].contiguous()
        U = torch.zeros_like(B)
        for _ in range(2):
            it, res = g.lod_solve_multi(values.data_ptr(), cols.data_ptr(), B.data_ptr(), n, n, U.data_ptr(), n, REL_TOL, 20000)
        print(json.dumps({"n_rhs": n, "iterations_max": int(it.max()), "solves": 2}))
        return

    for n in (1, 4, 16, 64, 256):
        B = Ball[:, :n].contiguous()
        U = torch.zeros_like(B)
        cols1 = [Ball[:, k].contiguous() for k in range(n)]
        u1 = torch.zeros(NP, dtype=torch.float64, device=dev)

        def multi():
            return g.lod_solve_multi(values.data_ptr(), cols.data_ptr(), B.data_ptr(), n, n, U.data_ptr(), n, REL_TOL, 20000)

        def singles():
            return [g.lod_solve(values.data_ptr(), cols.data_ptr(), c.data_ptr(), u1.data_ptr(), REL_TOL, 20000)[0]
                    for c in cols1]

        multi(), singles()                                                    # warm-up of both shapes
        tm = sorted(timed(multi)[:2] for _ in range(args.reps))[args.reps // 2]
        ts = sorted(timed(singles)[:2] for _ in range(args.reps))[args.reps // 2]
        it, res = multi()
        it1 = singles()
        itmax, bursts = int(it.max()), (int(it.max()) + 7) // 8
        # compulsory bytes of one product: values + cols of the used slots, one row of P per used slot, Y
        product_bytes = used * (8 + 4) + used * 8 * n + NP * 8 * n
        print(json.dumps({
            "n_rhs": n, "multi_event_ms": tm[0], "multi_wall_ms": tm[1], "multi_ms_per_column": tm[0] / n,
            "singles_event_ms": ts[0], "singles_wall_ms": ts[1], "singles_ms_per_column": ts[0] / n,
            "iterations_multi_max": itmax, "iterations_multi_mean": float(it.mean()),
            "iterations_single_mean": float(np.mean(it1)), "max_rel_residual": float(res.max()),
            "launches_per_iteration_multi": (3 * itmax + bursts) / max(itmax, 1), "launches_per_iteration_single": 4.0,
            "product_bytes_per_iteration": product_bytes,
            "product_GBps_lower_bound": product_bytes * itmax / (tm[0] * 1e-3) / 1e9,
            "used_slots": used}), flush=True)


if __name__ == "__main__":
    main()
