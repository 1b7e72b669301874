#!/usr/bin/env python3
"""Time the ensemble calls against K sequential single-problem calls on BASELINE configuration C2 (2-D Poisson,
H = 1/32, n_sub 8, oversampling 2: 1024 patches, 121 slots per block row), rel_tol 1e-10, in one process.

One handle with n_problems = 64, member k the D1e4 field of seed SEED + k, one plan over all 64 * 1024 bases; K = 1, 8,
64 take the first K members of that slab.  Per K, medians of --reps after a warm-up, HIP-event and host wall time:
  solve     slod_lod_solve_ensemble against K slod_lod_solve_multi(n_rhs = 1) calls on the de-interleaved matrices
            (copies made beforehand, outside the timing), with the iteration counts of both (they must agree);
  assemble  slod_lod_matrix_ensemble + slod_lod_rhs_ensemble + slod_lod_reconstruct_ensemble against K times
            slod_lod_matrix + slod_lod_rhs + slod_lod_reconstruct on the member slabs.
product_bytes_per_iteration is what one product Y_k = A_k P_k of all members must move: the values of the used slots of
every member, the columns once, one row of P per used slot and member, and Y; over the event time of the whole solve
it gives a lower bound of the product's rate (the solve also runs the two update kernels).  One JSON line per K.

  python tools/lod_ensemble_timing.py [--reps 5] [--members 1 8 64]
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
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64])
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_ensemble_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    kmax = max(args.members)
    g = slod_amd.Slod(n_problems=kmax, **C2)
    for k in range(kmax):
        t = torch.from_numpy(fill_coefficient(SEED + k, "D1e4", g.NE)).to(dev)
        g.set_coefficient_device(0, t.data_ptr(), t.numel(), problem=k)
        torch.cuda.synchronize()
    NP, cap = g.num_patches, g.lod_row_capacity()
    ids = np.arange(NP, dtype=np.uint32)
    plan = g.plan(np.arange(kmax * NP, dtype=np.uint32))
    stride, mstride = plan.stride, NP * plan.stride
    b = torch.zeros(kmax * mstride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    nfine, nval = (g.NE + 1) ** 2, NP * cap
    load = torch.zeros(nfine, dtype=torch.float64, device=dev)
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()

    def timed(fn):
        """(event ms, wall ms) of fn(); the events sit on the null stream, fn ends synchronised."""
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
        fn()                                                                  # warm-up
        return sorted(timed(fn) for _ in range(args.reps))[args.reps // 2]

    for K in args.members:
        V = torch.zeros(nval, K, dtype=torch.float64, device=dev)
        cols = torch.zeros(nval, dtype=torch.int32, device=dev)
        R = torch.zeros(NP, K, dtype=torch.float64, device=dev)
        U = torch.zeros_like(R)
        fine = torch.zeros(K, nfine, dtype=torch.float64, device=dev)
        v1 = torch.zeros(nval, dtype=torch.float64, device=dev)
        c1 = torch.zeros(nval, dtype=torch.int32, device=dev)
        r1 = torch.zeros(NP, dtype=torch.float64, device=dev)
        u1 = torch.zeros(NP, dtype=torch.float64, device=dev)
        f1 = torch.zeros(nfine, dtype=torch.float64, device=dev)

        def assemble_ens():
            g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), stride, K, V.data_ptr(), cols.data_ptr())
            g.lod_rhs_ensemble(b.data_ptr(), stride, K, load.data_ptr(), R.data_ptr())
            g.lod_reconstruct_ensemble(b.data_ptr(), stride, K, R.data_ptr(), fine.data_ptr())

        def assemble_seq():
            for k in range(K):
                bk, qk = b.data_ptr() + 8 * k * mstride, q.data_ptr() + 8 * k * mstride
                g.lod_matrix(ids, bk, qk, stride, v1.data_ptr(), c1.data_ptr())
                g.lod_rhs(ids, bk, stride, load.data_ptr(), r1.data_ptr())
                g.lod_reconstruct(bk, stride, r1.data_ptr(), f1.data_ptr())

        ta, tq = median(assemble_ens), median(assemble_seq)
        used = int((cols.cpu().numpy().view(np.uint32) != 0xffffffff).sum())
        Vk = [V[:, k].contiguous() for k in range(K)]
        Rk = [R[:, k].contiguous() for k in range(K)]
        out = {}

        def solve_ens():
            out["ens"] = g.lod_solve_ensemble(V.data_ptr(), cols.data_ptr(), R.data_ptr(), U.data_ptr(), K, rel_tol=REL_TOL,
                                              max_iterations=20000)

        def solve_seq():
            out["seq"] = [g.lod_solve_multi(Vk[k].data_ptr(), cols.data_ptr(), Rk[k].data_ptr(), 1, 1, u1.data_ptr(), 1, REL_TOL,
                                            20000)[0][0] for k in range(K)]

        ts, tr = median(solve_ens), median(solve_seq)
        it, res = out["ens"]
        itmax = int(it.max())
        product_bytes = used * 8 * K + used * 4 + used * 8 * K + NP * 8 * K
        print(json.dumps({
            "n_members": K, "solve_ensemble_event_ms": ts[0], "solve_ensemble_wall_ms": ts[1],
            "solve_sequential_event_ms": tr[0], "solve_sequential_wall_ms": tr[1], "solve_speedup_event": tr[0] / ts[0],
            "iterations_ensemble": it.tolist(), "iterations_sequential": [int(i) for i in out["seq"]],
            "iterations_agree": bool((it == np.array(out["seq"])).all()), "max_rel_residual": float(res.max()),
            "assemble_ensemble_event_ms": ta[0], "assemble_ensemble_wall_ms": ta[1],
            "assemble_sequential_event_ms": tq[0], "assemble_sequential_wall_ms": tq[1],
            "assemble_speedup_event": tq[0] / ta[0],
            "product_bytes_per_iteration": product_bytes,
            "product_GBps_lower_bound": product_bytes * itmax / (ts[0] * 1e-3) / 1e9, "used_slots": used}), flush=True)


if __name__ == "__main__":
    main()
